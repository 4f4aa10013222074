// Born modelling on the stores that do not hold every q^n in the field's type (fwi_born.h, second half): the weight of a
// strided store, the scatter pass that reads a bf16 store, and the amplitudes of the source's exact share.  Its own
// object: fwi_born.o keeps its pinned kernel count and register figures.
//
// The bf16 scatter is the bandwidth-bound pass of fwi_born.hip with a narrower q: per point and step it reads q (2 B,
// streaming: once per sweep, it must not evict the field), w (4 B) and read-modify-writes the padded field (8 B) --
// 14 B against the native store's 16.
#include <algorithm>

#include "fwi_born.h"
#include "fwi_device.h"

namespace fwi {

namespace {

constexpr int BORN_BLOCK = 256;

template <typename T>
__global__ __launch_bounds__(BORN_BLOCK) void born_weight_strided(const T *dm, const T *c, T *w, int wrt_velocity,
                                                                  double stride, int64_t n, int nx, int cx) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double v = 0.0;  // pad column (c = 0 there)
        if (cx == nx || (int)(i % cx) < nx) {
            const double cc = (double)c[i], d = (double)dm[i];
            v = stride * (wrt_velocity ? 2.0 * d / cc : -(cc * cc) * d);
        }
        w[i] = (T)v;
    }
}

// One thread per four points of the compact layout (rows of cx elements, cx % 4 == 0): a 16-byte vector of the field and
// of w, an 8-byte one of the store.  Element i of the store lies 2 i bytes in, so the 8-byte loads are aligned wherever
// the 16-byte ones are.
__global__ __launch_bounds__(BORN_BLOCK) void born_scatter_bf16(float *u, const void *q, const float *w, const float *dz,
                                                                const float *dy, const float *dx, int damp, GridDesc g,
                                                                int nvec) {
    const int i = blockIdx.x * BORN_BLOCK + threadIdx.x;
    if (i >= nvec) return;
    const int cxv = g.cx / 4;
    const int row = i / cxv, x0 = (i - row * cxv) * 4;
    const int z = row / g.ny, y = row - z * g.ny;
    const int64_t ci = (int64_t)row * g.cx + x0;
    const int64_t p = g.off0 + (int64_t)z * g.sz + (int64_t)y * g.sy + x0;
    const f4 qv = ld_bf16x4_stream(q, ci);
    const f4 wv = ld4(w + ci);
    f4 uv = ld4(u + p);
    float dzv = 0.f, dyv = 0.f;
    if (damp) {
        dzv = dz[z];
        dyv = dy[y];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + j;
        if (x >= g.nx) continue;  // pad column: a halo cell of the padded field, stays zero
        float add = wv.v[j] * qv.v[j];
        if (damp) add = add / (1.f + (dzv + dx[x] + dyv));  // (the order of fwi_born.hip's sum)
        uv.v[j] += add;
    }
    st4(u + p, uv);
}

__global__ __launch_bounds__(BORN_BLOCK) void born_source_share(const float *w, const int64_t *cidx, const float *wav,
                                                                float *out, int n, int nsrc) {
    const int i = blockIdx.x * BORN_BLOCK + threadIdx.x;
    if (i < n) out[i] = w[cidx[i % nsrc]] * wav[i];
}

}  // namespace

template <typename T>
hipError_t launch_born_weight_strided(const GridDesc &g, const T *dm, const T *c, T *w, int wrt_velocity, int stride,
                                      hipStream_t s) {
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(2048, (g.npts + BORN_BLOCK - 1) / BORN_BLOCK));
    hipLaunchKernelGGL(born_weight_strided<T>, dim3(blocks), dim3(BORN_BLOCK), 0, s, dm, c, w, wrt_velocity, (double)stride,
                       g.npts, g.nx, g.cx);
    return hipGetLastError();
}

hipError_t launch_born_scatter_bf16(const GridDesc &g, float *u, const void *q_bf16, const float *w, const float *dz,
                                    const float *dy, const float *dx, int damp, hipStream_t s) {
    if (g.ndim != 3) return hipErrorInvalidValue;  // (the bf16 store exists for 3-D contexts only)
    const int64_t nvec = g.npts / 4;
    if (nvec <= 0) return hipSuccess;
    if (nvec > (int64_t)0x7fffffff - BORN_BLOCK) return hipErrorInvalidValue;
    const int blocks = (int)((nvec + BORN_BLOCK - 1) / BORN_BLOCK);
    hipLaunchKernelGGL(born_scatter_bf16, dim3(blocks), dim3(BORN_BLOCK), 0, s, u, q_bf16, w, dz, dy, dx, damp, g, (int)nvec);
    return hipGetLastError();
}

hipError_t launch_born_source_share(const float *w, const int64_t *cidx, const float *wav, float *out, int nt, int nsrc,
                                    hipStream_t s) {
    const int64_t n = (int64_t)nt * nsrc;
    if (n <= 0) return hipSuccess;
    if (n > (int64_t)0x7fffffff - BORN_BLOCK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(born_source_share, dim3((unsigned)((n + BORN_BLOCK - 1) / BORN_BLOCK)), dim3(BORN_BLOCK), 0, s, w, cidx,
                       wav, out, (int)n, nsrc);
    return hipGetLastError();
}

template hipError_t launch_born_weight_strided<float>(const GridDesc &, const float *, const float *, float *, int, int,
                                                      hipStream_t);
template hipError_t launch_born_weight_strided<double>(const GridDesc &, const double *, const double *, double *, int, int,
                                                       hipStream_t);

}  // namespace fwi
