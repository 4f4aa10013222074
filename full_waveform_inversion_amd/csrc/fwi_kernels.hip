// gfx950 (MI355X, CDNA4) kernels of the acoustic time-stepping path.
//
// No reference counterpart: the reference has no stencil / PML / adjoint /
// imaging code; the scheme is the build-defined one stated at
// the top of oracle/fwi_oracle.py.  All kernels are HBM-bandwidth bound
// (~2.4 flop/B), so no MFMA: the work here is coalesced 16 B/lane streams,
// an LDS-staged xy halo tile, a register queue along z and wave64 shuffles
// for the reductions.
//
// Numerics: the Laplacian is evaluated in difference form
//     L u = sum_k c_k * ( sum_axes (u[+k] + u[-k]) - 2 D u )
// which is algebraically the centred star but keeps fp32 round-off ~30x lower
// over thousands of steps than the coefficient form (the rounded coefficients
// of the latter do not sum to zero, which acts as a spurious mass term).
#include "fwi_device.h"

namespace fwi {

// ---------------------------------------------------------------------------
// POINT kernel: one thread per grid point, all 4r+... neighbours straight from
// global memory (L1/L2 absorb the re-reads).  Generic in dtype, order and
// dimension; the fallback for shapes the stream kernel does not take and the
// on-device cross-check of it.
// ---------------------------------------------------------------------------
template <typename T, int R, int NDIM, bool SAVE_Q, bool IMAGE, bool INC>
__global__ __launch_bounds__(256) void step_point(StepArgs<T> a, GridDesc g, int nbx, int nby, int nblk) {
    const int tid = threadIdx.y * 64 + threadIdx.x;
    if ((int)blockIdx.x >= nblk) {
        // receiver sampling of the previous step's field (u_cur) rides along as extra workgroups
        for (int i = ((int)blockIdx.x - nblk) * 256 + tid; i < a.nrec; i += ((int)gridDim.x - nblk) * 256)
            a.rec_out[i] = a.u_cur[a.rec_pidx[i]] * a.rec_scale;
        return;
    }
    // (the host's side of this decode: point_tile_of, fwi_points.cpp)
    const int bx = blockIdx.x % nbx;
    const int t2 = blockIdx.x / nbx;
    const int x = bx * 64 + threadIdx.x;
    int y, z;
    if (NDIM == 3) {
        y = (t2 % nby) * 4 + threadIdx.y;
        z = t2 / nby;
    } else {
        y = 0;
        z = t2 * 4 + threadIdx.y;
    }
    if (x < g.nx && y < g.ny && z < g.nz) {
        const int64_t p = g.off0 + (int64_t)z * g.sz + (int64_t)y * g.sy + x;
        const T *u = a.u_cur + p;
        const T uc = u[0];
        T lap = T(0);
#pragma unroll
        for (int k = R; k >= 1; --k) {
            T t = (u[-k] + u[k]) + (u[-(int64_t)k * g.sz] + u[(int64_t)k * g.sz]);
            if (NDIM == 3) t += (u[-(int64_t)k * g.sy] + u[(int64_t)k * g.sy]);
            t = fma(T(-2 * NDIM), uc, t);
            lap = fma(a.ck[k], t, lap);
        }
        if (NDIM == 3 && a.pml_tz) {  // the z / y border's CPML term, handed over by the line launch before this step
            if (pml_in_shell(z, g.nz, a.npml, R))
                lap += a.pml_tz[((int64_t)pml_shell_index(z, g.nz, a.npml, R) * g.ny + y) * g.cx + x];
            if (pml_in_shell(y, g.ny, a.npml, R))
                lap += a.pml_ty[((int64_t)z * pml_shell_rows(g.ny, a.npml, R) + pml_shell_index(y, g.ny, a.npml, R)) * g.cx + x];
        }
        const T q = a.C[p] * lap;
        const T up = INC ? a.v[p] : a.u_prev[p];  // increment form: the operand is v^n = u^n - u^{n-1}
        T un;
        if (a.damp) {
            T d = a.dz[z] + a.dx[x];
            if (NDIM == 3) d += a.dy[y];
            if (INC) {
                const T vn = ((T(1) - d) * up + q) / (T(1) + d);
                a.v[p] = vn;
                un = uc + vn;
            } else {
                un = (T(2) * uc - (T(1) - d) * up + q) / (T(1) + d);
            }
        } else if (INC) {
            const T vn = up + q;
            a.v[p] = vn;
            un = uc + vn;
        } else {
            un = (T(2) * uc - up) + q;
        }
        a.u_prev[p] = un;
        const int64_t ci = ((int64_t)z * g.ny + y) * g.cx + x;
        if (SAVE_Q) a.q_out[ci] = q;
        // (paired imaging: the second pairing takes u_prev -- in increment form u - v, `up` being v there)
        if (IMAGE) a.g[ci] += a.q_in2 ? fma(INC ? uc - up : up, a.q_in2[ci], uc * a.q_in[ci]) : uc * a.q_in[ci];
    }
    // injection into the points this workgroup has just written (see the stream kernel)
    if (a.inj_start) {
        const int s0 = a.inj_start[blockIdx.x], s1 = a.inj_start[blockIdx.x + 1];
        if (s1 > s0) {
            __syncthreads();
            inject_runs<T, INC, SAVE_Q>(a, s0, s1, tid, 256);
        }
    }
}

constexpr int TILE_X = 256;                // 2-D tile kernel: floats per tile row = 64 lanes x float4
constexpr int LROW4 = TILE_X / 4 + 2;      // its LDS row in float4: [left edge][64][right edge]

// ---------------------------------------------------------------------------
// TILE kernel (2-D, fp32): the 2-D sibling of the stream kernel.  A workgroup of 64 x TY threads
// owns a 256 x TY (x, z) tile, one float4 per thread; the TY + 2r rows it needs are staged in LDS
// once (one barrier), x neighbours come from the same LDS row.  2-D grids of BASELINE size are
// L2-resident (1024^2: 4 MiB per field), so a time step is bounded by the ~1.5 us kernel boundary
// plus one load -> barrier -> compute -> store chain; there is no marching axis to pipeline.
// ---------------------------------------------------------------------------
template <int R, int TY, bool DAMP, bool SAVE_Q, int IMAGE>
__global__ __launch_bounds__(64 * TY) void step2d_tile(StepArgs<float> a, GridDesc g, int nxt, int nblk) {
    constexpr int NH = (2 * R + TY - 1) / TY;
    constexpr int TRASH = TY + 2 * R;
    constexpr int LROWS = TY + 2 * R + 1;
    __shared__ f4 L[LROWS][LROW4];

    const int lane = threadIdx.x, ty = threadIdx.y;
    int bid = blockIdx.x;
    if (bid >= nblk) {  // receiver sampling of the previous step's field
        for (int i = (bid - nblk) * (64 * TY) + ty * 64 + lane; i < a.nrec; i += (gridDim.x - nblk) * 64 * TY)
            a.rec_out[i] = a.u_cur[a.rec_pidx[i]] * a.rec_scale;
        return;
    }
    const int bx = bid % nxt, bz = bid / nxt;  // (the host's side of this decode: stream_tile_of, fwi_points.cpp)
    const int x0 = bx * TILE_X + 4 * lane;
    const int z0 = bz * TY, z = z0 + ty;
    const bool act = (x0 < g.nx) && (z < g.nz);
    const int64_t sz = g.sz;
    const int xa = min(x0, ((g.nx - 1) / 4 + 1) * 4);  // lanes right of the grid read one shared zero vector
    const int64_t poff = g.off0 + (int64_t)z * sz + xa;

    const f4 ctr = ld4(a.u_cur + poff);
    f4 halo[NH];
    int hrow[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        const int hr = ty + i * TY;
        const bool valid = hr < 2 * R;
        const int zh = !valid ? z : (hr < R) ? z0 - R + hr : z0 + TY + (hr - R);
        hrow[i] = !valid ? TRASH : (hr < R) ? hr : TY + hr;
        halo[i] = ld4(a.u_cur + g.off0 + (int64_t)zh * sz + xa);
    }
    const int64_t rowoff = g.off0 + (int64_t)z * sz + bx * TILE_X;
    const int64_t eoff = (lane < 4) ? rowoff - 4 + lane : (lane >= 60) ? rowoff + TILE_X + (lane - 60) : rowoff - 1;
    const int erow = (lane < 4 || lane >= 60) ? R + ty : TRASH;
    const int ecol = (lane < 4) ? lane : (lane >= 60) ? 4 * (LROW4 - 1) + (lane - 60) : lane;
    const float edge = a.u_cur[eoff];
    const f4 up = ld4(a.u_prev + poff), Cc = ld4(a.C + poff);
    const int64_t ci = (int64_t)z * g.cx + x0;
    f4 qi, qi2, gi;
    if (IMAGE) {
        qi = ld4_stream(a.q_in + (act ? ci : 0));
        if (IMAGE == 2) qi2 = ld4_stream(a.q_in2 + (act ? ci : 0));
        gi = ld4(a.g + (act ? ci : 0));
    }
    f4 A, B;
    if (DAMP) {
        const float dzv = (z < g.nz) ? a.dz[z] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float d = dzv + ((x0 + j < g.nx) ? a.dx[x0 + j] : 0.f);
            B.v[j] = 1.f - d;
            A.v[j] = rcp_nr(1.f + d);
        }
    }

    L[R + ty][1 + lane] = ctr;
#pragma unroll
    for (int i = 0; i < NH; ++i) L[hrow[i]][1 + lane] = halo[i];
    reinterpret_cast<float *>(&L[erow][0])[ecol] = edge;
    __syncthreads();

    const f4 xl = L[R + ty][lane], xr = L[R + ty][lane + 2];
    float X[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        X[j] = xl.v[j];
        X[4 + j] = ctr.v[j];
        X[8 + j] = xr.v[j];
    }
    f4 lap;
#pragma unroll
    for (int j = 0; j < 4; ++j) lap.v[j] = 0.f;
#pragma unroll
    for (int k = R; k >= 1; --k) {
        const f4 zm = L[R + ty - k][1 + lane], zp = L[R + ty + k][1 + lane];
        const float c = a.ck[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float t = (X[4 + j - k] + X[4 + j + k]) + (zm.v[j] + zp.v[j]);
            t = fmaf(-4.f, X[4 + j], t);
            lap.v[j] = fmaf(c, t, lap.v[j]);
        }
    }
    f4 q, un;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q.v[j] = Cc.v[j] * lap.v[j];
        if (DAMP)
            un.v[j] = (fmaf(2.f, X[4 + j], -B.v[j] * up.v[j]) + q.v[j]) * A.v[j];
        else
            un.v[j] = (2.f * X[4 + j] - up.v[j]) + q.v[j];
    }
    if (act) {
        st4(a.u_prev + poff, un);
        if (SAVE_Q) st4_stream(a.q_out + ci, q);
        if (IMAGE) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                gi.v[j] = fmaf(X[4 + j], qi.v[j], gi.v[j]);
                if (IMAGE == 2) gi.v[j] = fmaf(up.v[j], qi2.v[j], gi.v[j]);
            }
            st4(a.g + ci, gi);
        }
    }
    if (a.inj_start) {  // injection into the points this workgroup has just written
        const int s0 = a.inj_start[bid], s1 = a.inj_start[bid + 1];
        if (s1 > s0) {
            __syncthreads();
            inject_runs<float, false, SAVE_Q>(a, s0, s1, ty * 64 + lane, 64 * TY);
        }
    }
}

template <typename T>
static hipError_t launch_stream(const GridDesc &g, const StepArgs<T> &a, const StreamTuning &t, hipStream_t s) {
    switch (g.r) {
        case 1: return launch_stream_r<T, 1>(g, a, t, s);
        case 2: return launch_stream_r<T, 2>(g, a, t, s);
        default: return launch_stream_r<T, 4>(g, a, t, s);
    }
}

template <int R, int TY, bool DAMP>
static hipError_t launch_tile2d_mode(const GridDesc &g, const StepArgs<float> &a, hipStream_t s) {
    const int nxt = stream_nxt(g, TILE_X);
    const int nblk = nxt * ((g.nz + TY - 1) / TY);
    const int nrb = (a.rec_out && a.nrec > 0) ? (a.nrec + 64 * TY * 4 - 1) / (64 * TY * 4) : 0;
    dim3 block(64, TY), grid(nblk + nrb);
    if (a.q_out)
        hipLaunchKernelGGL((step2d_tile<R, TY, DAMP, true, 0>), grid, block, 0, s, a, g, nxt, nblk);
    else if (a.q_in && a.q_in2)
        hipLaunchKernelGGL((step2d_tile<R, TY, DAMP, false, 2>), grid, block, 0, s, a, g, nxt, nblk);
    else if (a.q_in)
        hipLaunchKernelGGL((step2d_tile<R, TY, DAMP, false, 1>), grid, block, 0, s, a, g, nxt, nblk);
    else
        hipLaunchKernelGGL((step2d_tile<R, TY, DAMP, false, 0>), grid, block, 0, s, a, g, nxt, nblk);
    return hipGetLastError();
}

template <int R>
static hipError_t launch_tile2d_r(const GridDesc &g, const StepArgs<float> &a, const StreamTuning &t,
                                  hipStream_t s) {
    if (a.damp) {
        switch (t.ty) {
            case 4: return launch_tile2d_mode<R, 4, true>(g, a, s);
            case 16: return launch_tile2d_mode<R, 16, true>(g, a, s);
            default: return launch_tile2d_mode<R, 8, true>(g, a, s);
        }
    }
    switch (t.ty) {
        case 4: return launch_tile2d_mode<R, 4, false>(g, a, s);
        case 16: return launch_tile2d_mode<R, 16, false>(g, a, s);
        default: return launch_tile2d_mode<R, 8, false>(g, a, s);
    }
}

static inline void point_blocks(const GridDesc &g, int &nbx, int &nby, int &nblk) {
    nbx = (g.nx + 63) / 64;
    nby = (g.ndim == 3) ? (g.ny + 3) / 4 : (g.nz + 3) / 4;
    nblk = nbx * nby * ((g.ndim == 3) ? g.nz : 1);
}

template <typename T, int R, int NDIM>
static hipError_t launch_point_mode(const GridDesc &g, const StepArgs<T> &a, hipStream_t s) {
    int nbx, nby, nblk;
    point_blocks(g, nbx, nby, nblk);
    const int nrb = (a.rec_out && a.nrec > 0) ? (a.nrec + 1023) / 1024 : 0;
    dim3 block(64, 4), grid(nblk + nrb);
    if (a.v) {
        if (a.q_out)
            hipLaunchKernelGGL((step_point<T, R, NDIM, true, false, true>), grid, block, 0, s, a, g, nbx, nby, nblk);
        else if (a.q_in)
            hipLaunchKernelGGL((step_point<T, R, NDIM, false, true, true>), grid, block, 0, s, a, g, nbx, nby, nblk);
        else
            hipLaunchKernelGGL((step_point<T, R, NDIM, false, false, true>), grid, block, 0, s, a, g, nbx, nby, nblk);
    } else if (a.q_out)
        hipLaunchKernelGGL((step_point<T, R, NDIM, true, false, false>), grid, block, 0, s, a, g, nbx, nby, nblk);
    else if (a.q_in)
        hipLaunchKernelGGL((step_point<T, R, NDIM, false, true, false>), grid, block, 0, s, a, g, nbx, nby, nblk);
    else
        hipLaunchKernelGGL((step_point<T, R, NDIM, false, false, false>), grid, block, 0, s, a, g, nbx, nby, nblk);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_point(const GridDesc &g, const StepArgs<T> &a, hipStream_t s) {
    if (g.ndim == 3) {
        switch (g.r) {
            case 1: return launch_point_mode<T, 1, 3>(g, a, s);
            case 2: return launch_point_mode<T, 2, 3>(g, a, s);
            default: return launch_point_mode<T, 4, 3>(g, a, s);
        }
    }
    switch (g.r) {
        case 1: return launch_point_mode<T, 1, 2>(g, a, s);
        case 2: return launch_point_mode<T, 2, 2>(g, a, s);
        default: return launch_point_mode<T, 4, 2>(g, a, s);
    }
}

template <>
hipError_t launch_step<float>(int kernel, const GridDesc &g, const StepArgs<float> &a,
                              const StreamTuning &t, hipStream_t s) {
    if (kernel == K_STREAM && g.ndim == 2) {
        switch (g.r) {
            case 1: return launch_tile2d_r<1>(g, a, t, s);
            case 2: return launch_tile2d_r<2>(g, a, t, s);
            default: return launch_tile2d_r<4>(g, a, t, s);
        }
    }
    if (kernel == K_STREAM) return launch_stream<float>(g, a, t, s);
    return launch_point<float>(g, a, s);
}

template <>
hipError_t launch_step<double>(int kernel, const GridDesc &g, const StepArgs<double> &a, const StreamTuning &t,
                               hipStream_t s) {
    if (kernel == K_STREAM && g.ndim == 3) return launch_stream<double>(g, a, t, s);
    return launch_point<double>(g, a, s);
}

// ---------------------------------------------------------------------------
// Receiver sampling of the final step (earlier steps are sampled inside the step launches).
// ---------------------------------------------------------------------------
template <typename T>
__global__ void record_kernel(const T *u, const int64_t *pidx, T *out, T scale, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = u[pidx[i]] * scale;
}

template <typename T>
hipError_t launch_record(const T *u, const int64_t *pidx, T *out, T scale, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(record_kernel<T>, dim3((n + 63) / 64), dim3(64), 0, s, u, pidx, out, scale, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Imaging tail, gradient scaling, dot product.
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T q_elem(const T *q, int64_t i, int bf16) {
    if (bf16) return (T)__uint_as_float((unsigned)reinterpret_cast<const unsigned short *>(q)[i] << 16);
    return q[i];
}

// g[x_s] += sum_n mu^{n+1}(x_s) * cq_s * w^n_s: the part of the imaging term that is the source itself (bf16 store).
// One thread per NODE, over the copy of the source set sorted by node (step_table, fwi_points.h: the entries of a node are consecutive,
// `run` holds their number at the first of them and 0 at the others, `col` the entry's column of the series): the shares
// of the sources that sit on one node are added in that order, as the injection adds them, and by a plain store -- an
// atomicAdd per source left the order of two such sources, and with it the last bit of the gradient there, to the hardware.
template <typename T>
__global__ void source_image_kernel(const T *adj_series, const T *wav, const int64_t *s_cidx, const T *s_cq,
                                    const int *s_col, const int *s_run, T *gacc, int nt, int nsrc, int stride, T inv_rs) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nsrc) return;
    const int len = s_run[k];
    if (len == 0) return;
    T g = gacc[s_cidx[k]];
    for (int j = k; j < k + len; ++j) {
        const int sidx = s_col[j];
        double acc = 0.0;
        for (int n = 0; n < nt; n += stride)
            acc += (double)adj_series[(int64_t)n * nsrc + sidx] * (double)wav[(int64_t)n * nsrc + sidx];
        g += (T)(acc * (double)inv_rs * (double)s_cq[j]);
    }
    gacc[s_cidx[k]] = g;
}

template <typename T>
hipError_t launch_source_image(const T *adj_series, const T *wav, const int64_t *s_cidx, const T *s_cq, const int *s_col,
                               const int *s_run, T *gacc, int nt, int nsrc, int stride, T inv_rs, hipStream_t s) {
    if (nsrc <= 0) return hipSuccess;
    hipLaunchKernelGGL(source_image_kernel<T>, dim3((nsrc + 63) / 64), dim3(64), 0, s, adj_series, wav, s_cidx, s_cq, s_col,
                       s_run, gacc, nt, nsrc, stride, inv_rs);
    return hipGetLastError();
}

template <typename T>
__global__ void image_kernel(GridDesc g, const T *u, const T *q, T *gacc, int q_bf16) {
    const int64_t rowlen = g.cx;
    for (int64_t ci = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; ci < g.npts;
         ci += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = ci / rowlen;  // z * ny + y
        const int x = (int)(ci - row * rowlen);
        if (x >= g.nx) continue;  // pad column of the compact layout
        const int z = (int)(row / g.ny), y = (int)(row % g.ny);
        const int64_t p = g.off0 + (int64_t)z * g.sz + (int64_t)y * g.sy + x;
        gacc[ci] += u[p] * q_elem<T>(q, ci, q_bf16);
    }
}

template <typename T>
hipError_t launch_image(const GridDesc &g, const T *u, const T *q, T *gacc, int q_bf16, hipStream_t s) {
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(4096, (g.npts + 255) / 256));
    hipLaunchKernelGGL(image_kernel<T>, dim3(blocks), dim3(256), 0, s, g, u, q, gacc, q_bf16);
    return hipGetLastError();
}

// padded C = dt^2 c^2 from the compact velocity; counts non-finite / non-positive entries in *bad
template <typename T>
__global__ void build_model_kernel(GridDesc g, const T *c, T *Cpad, double dt2, int *bad) {
    for (int64_t ci = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; ci < g.npts;
         ci += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = ci / g.cx;
        const int x = (int)(ci - row * g.cx);
        if (x >= g.nx) continue;  // pad column: C stays 0 there, which freezes u at 0 (a Dirichlet wall)
        const int z = (int)(row / g.ny), y = (int)(row % g.ny);
        const double cv = (double)c[ci];
        if (!(cv > 0.0) || !isfinite(cv)) atomicAdd(bad, 1);
        Cpad[g.off0 + (int64_t)z * g.sz + (int64_t)y * g.sy + x] = (T)(dt2 * cv * cv);
    }
}

template <typename T>
hipError_t launch_build_model(const GridDesc &g, const T *c, T *Cpad, double dt2, int *bad, hipStream_t s) {
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(4096, (g.npts + 255) / 256));
    hipLaunchKernelGGL(build_model_kernel<T>, dim3(blocks), dim3(256), 0, s, g, c, Cpad, dt2, bad);
    return hipGetLastError();
}

template <typename T>
__global__ void finalize_gradient_kernel(const T *gacc, const T *c, T *out, double scale,
                                         int wrt_velocity, int64_t n, int nx, int cx) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        double v = (double)gacc[i] * scale;
        if (wrt_velocity) {
            const double cc = (double)c[i];
            v *= -2.0 / (cc * cc * cc);
        }
        if (cx != nx && (int)(i % cx) >= nx) v = 0.0;  // pad column (c = 0 there)
        out[i] = (T)v;
    }
}

template <typename T>
hipError_t launch_finalize_gradient(const GridDesc &g, const T *gacc, const T *c, T *out, double scale,
                                    int wrt_velocity, hipStream_t s) {
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (g.npts + 255) / 256));
    hipLaunchKernelGGL(finalize_gradient_kernel<T>, dim3(blocks), dim3(256), 0, s, gacc, c, out, scale,
                       wrt_velocity, g.npts, g.nx, g.cx);
    return hipGetLastError();
}

// compact (stride cx, pad columns zeroed) <-> contiguous (stride nx)
template <typename T>
__global__ void repack_kernel(T *dst, const T *src, int64_t rows, int nx, int cx, int to_compact) {
    const int64_t n = rows * cx;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / cx;
        const int x = (int)(i - row * cx);
        if (to_compact)
            dst[i] = x < nx ? src[row * nx + x] : T(0);
        else if (x < nx)
            dst[row * nx + x] = src[i];
    }
}

template <typename T>
hipError_t launch_repack(const GridDesc &g, T *dst, const T *src, int to_compact, hipStream_t s) {
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(4096, (g.npts + 255) / 256));
    hipLaunchKernelGGL(repack_kernel<T>, dim3(blocks), dim3(256), 0, s, dst, src, (int64_t)g.nz * g.ny, g.nx, g.cx,
                       to_compact);
    return hipGetLastError();
}

// cells of a padded field outside the interior that are not exactly zero (NaN counts)
template <typename T>
__global__ void dirty_padding_kernel(GridDesc g, const T *f, unsigned long long *bad) {
    const int hy = g.ndim == 3 ? HALO : 0;
    unsigned long long n = 0;
    for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < g.ptot; p += (int64_t)gridDim.x * blockDim.x) {
        // interior cell (z, y, x) lives at off0 + z sz + y sy + x with off0 = HALO sz + hy sy + HALO: shift by the x halo
        const int64_t q = p - HALO;
        bool interior = false;
        if (q >= 0) {
            const int64_t zz = q / g.sz, r = q - zz * g.sz, yy = r / g.sy, xx = r - yy * g.sy;
            interior = zz >= HALO && zz < HALO + g.nz && yy >= hy && yy < hy + g.ny && xx < g.nx;
        }
        if (!interior && !(f[p] == T(0))) ++n;
    }
    if (n) atomicAdd(bad, n);
}

template <typename T>
hipError_t launch_count_dirty_padding(const GridDesc &g, const T *f, unsigned long long *bad, hipStream_t s) {
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(4096, (g.ptot + 255) / 256));
    hipLaunchKernelGGL(dirty_padding_kernel<T>, dim3(blocks), dim3(256), 0, s, g, f, bad);
    return hipGetLastError();
}

// The two sums of the optimiser and the misfit, in one fixed order: per thread over its ascending grid-stride indices
// (fp64 accumulator, starting from +0), the wave's shuffle tree (offsets 32, 16, .., 1), the four waves as
// (w0 + w1) + (w2 + w3) into part[block], and launch_sum_partials over the block partials (fwi_reg.hip: thread t adds
// part[t], part[t + 256], .. in ascending order, then a halving tree over the 256 threads) into part[blocks].  No
// floating-point atomics: equal inputs give equal bits on every call, context and rank.  tests/_vecops.py restates the
// order in NumPy.
__device__ inline void block_sum_to_partial(double acc, double *part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ double wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

template <typename T>
__global__ __launch_bounds__(256) void dot_kernel(const T *a, const T *b, int64_t n, double *part) {
    double acc = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x)
        acc += (double)a[i] * (double)b[i];
    block_sum_to_partial(acc, part);
}

int sum_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(SUM_MAX_BLOCKS, (n + 255) / 256)); }

template <typename T>
hipError_t launch_dot(const T *a, const T *b, int64_t n, double *part, hipStream_t s) {
    const int blocks = sum_blocks(n);
    hipLaunchKernelGGL(dot_kernel<T>, dim3(blocks), dim3(256), 0, s, a, b, n, part);
    hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_sum_partials(part, blocks, s);
}

// Least-squares residual and misfit on the device: r = syn - obs (written over obs, where the adjoint
// sweep reads its injection amplitudes), and the sum of r^2 in the order of dot_kernel.
template <typename T>
__global__ __launch_bounds__(256) void residual_l2_kernel(const T *syn, T *obs_inout, int64_t n, double *part) {
    double acc = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const T r = syn[i] - obs_inout[i];
        obs_inout[i] = r;
        acc += (double)r * (double)r;
    }
    block_sum_to_partial(acc, part);
}

template <typename T>
hipError_t launch_residual_l2(const T *syn, T *obs_inout, int64_t n, double *part, hipStream_t s) {
    const int blocks = sum_blocks(n);
    hipLaunchKernelGGL(residual_l2_kernel<T>, dim3(blocks), dim3(256), 0, s, syn, obs_inout, n, part);
    hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_sum_partials(part, blocks, s);
}

// Off-grid points (multilinear interpolation): per-point time series <-> per-node time series on the device.
//   scatter  node[n, m] = w[m] * point[n, owner[m]]                      (injection amplitudes)
//   gather   point[n, p] = sum_{m in nodes(p)} w[m] * node[n, m]         (sampling; the transpose)
// gather: a point has at most 2^D <= 8 nodes, so 8 lanes own one (time sample, point) pair and reduce with
// __shfl_down within their group of 8 -- the "wavefront reduction for the receiver gather" of north_star.
template <typename T>
__global__ void scatter_series_kernel(const T *pt, T *node, const int *owner, const T *w, int nt, int npts, int nnodes) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= (int64_t)nt * nnodes) return;
    const int n = (int)(i / nnodes), m = (int)(i - (int64_t)n * nnodes);
    node[i] = w[m] * pt[(int64_t)n * npts + owner[m]];
}

template <typename T>
__global__ __launch_bounds__(256) void gather_series_kernel(const T *node, T *pt, const int *pt_start, const T *w, int nt,
                                                            int npts, int nnodes) {
    const int64_t pair = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 3;  // (n, p), 8 lanes each
    const int sub = threadIdx.x & 7;
    T v = T(0);
    const bool live = pair < (int64_t)nt * npts;
    int n = 0, p = 0;
    if (live) {
        n = (int)(pair / npts);
        p = (int)(pair - (int64_t)n * npts);
        const int m = pt_start[p] + sub;
        if (m < pt_start[p + 1]) v = w[m] * node[(int64_t)n * nnodes + m];
    }
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) v += __shfl_down(v, off, 8);
    if (live && sub == 0) pt[pair] = v;
}

template <typename T>
hipError_t launch_scatter_series(const T *pt, T *node, const int *owner, const T *w, int nt, int npts, int nnodes,
                                 hipStream_t s) {
    const int64_t tot = (int64_t)nt * nnodes;
    if (tot <= 0) return hipSuccess;
    hipLaunchKernelGGL(scatter_series_kernel<T>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, pt, node, owner, w,
                       nt, npts, nnodes);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_gather_series(const T *node, T *pt, const int *pt_start, const T *w, int nt, int npts, int nnodes,
                                hipStream_t s) {
    const int64_t tot = (int64_t)nt * npts * 8;
    if (tot <= 0) return hipSuccess;
    hipLaunchKernelGGL(gather_series_kernel<T>, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, node, pt, pt_start,
                       w, nt, npts, nnodes);
    return hipGetLastError();
}

// Model-sized vector algebra for the optimiser (device-resident L-BFGS state).
template <typename T>
__global__ void axpby_kernel(T *y, double a, const T *x, double b, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = (T)(a * (double)x[i] + b * (double)y[i]);
}

template <typename T>
__global__ void clip_kernel(T *x, double lo, double hi, int64_t n, int nx, int cx) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (cx == nx || (int)(i % cx) < nx) {
            // NumPy's clip: only a value below lo or above hi is replaced, so a NaN stays and a zero that ties with a
            // bound of the other sign keeps its own sign
            const double v = (double)x[i];
            if (v < lo)
                x[i] = (T)lo;
            else if (v > hi)
                x[i] = (T)hi;
        }
}

// *out = max(*out, max |x|) as NumPy's np.abs(x).max(): a NaN wins over everything, +inf over every number.  wave64
// shuffle max, LDS across waves, one atomic per block.  The bit pattern of a non-negative double orders like an unsigned
// integer, and that of a positive NaN (fabs clears the sign) lies above +inf's: the integer atomic propagates the NaN and
// does not depend on the order of arrival.
__device__ inline double nan_max(double a, double b) { return (a != a || a > b) ? a : b; }  // b if b is NaN, too

template <typename T>
__global__ __launch_bounds__(256) void absmax_kernel(const T *x, int64_t n, unsigned long long *out) {
    double m = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        m = nan_max(fabs((double)x[i]), m);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = nan_max(m, __shfl_down(m, off, 64));
    __shared__ double part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = nan_max(nan_max(part[0], part[1]), nan_max(part[2], part[3]));
        atomicMax(out, (unsigned long long)__double_as_longlong(m));
    }
}

static inline int vec_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(2048, (n + 255) / 256)); }

template <typename T>
hipError_t launch_axpby(T *y, double a, const T *x, double b, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(axpby_kernel<T>, dim3(vec_blocks(n)), dim3(256), 0, s, y, a, x, b, n);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_clip(const GridDesc &g, T *x, double lo, double hi, hipStream_t s) {
    hipLaunchKernelGGL(clip_kernel<T>, dim3(vec_blocks(g.npts)), dim3(256), 0, s, x, lo, hi, g.npts, g.nx, g.cx);
    return hipGetLastError();
}
template <typename T>
hipError_t launch_absmax(const T *x, int64_t n, double *out, hipStream_t s) {
    hipLaunchKernelGGL(absmax_kernel<T>, dim3(vec_blocks(n)), dim3(256), 0, s, x, n, (unsigned long long *)out);
    return hipGetLastError();
}

#define FWI_INSTANTIATE(T)                                                                          \
    template hipError_t launch_record<T>(const T *, const int64_t *, T *, T, int, hipStream_t);    \
    template hipError_t launch_image<T>(const GridDesc &, const T *, const T *, T *, int, hipStream_t); \
    template hipError_t launch_source_image<T>(const T *, const T *, const int64_t *, const T *, const int *, const int *, \
                                               T *, int, int, int, T, hipStream_t);                 \
    template hipError_t launch_finalize_gradient<T>(const GridDesc &, const T *, const T *, T *, double, int, \
                                                    hipStream_t);                                  \
    template hipError_t launch_repack<T>(const GridDesc &, T *, const T *, int, hipStream_t);       \
    template hipError_t launch_dot<T>(const T *, const T *, int64_t, double *, hipStream_t);         \
    template hipError_t launch_count_dirty_padding<T>(const GridDesc &, const T *, unsigned long long *, hipStream_t); \
    template hipError_t launch_residual_l2<T>(const T *, T *, int64_t, double *, hipStream_t);       \
    template hipError_t launch_scatter_series<T>(const T *, T *, const int *, const T *, int, int, int, hipStream_t); \
    template hipError_t launch_gather_series<T>(const T *, T *, const int *, const T *, int, int, int, hipStream_t);  \
    template hipError_t launch_build_model<T>(const GridDesc &, const T *, T *, double, int *, hipStream_t); \
    template hipError_t launch_axpby<T>(T *, double, const T *, double, int64_t, hipStream_t);         \
    template hipError_t launch_clip<T>(const GridDesc &, T *, double, double, hipStream_t);           \
    template hipError_t launch_absmax<T>(const T *, int64_t, double *, hipStream_t);
FWI_INSTANTIATE(float)
FWI_INSTANTIATE(double)

}  // namespace fwi
