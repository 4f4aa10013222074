// Robust (Huber, hybrid L1/L2, Cauchy) data misfits and the median of |e| of (nt, ntr) trace gathers (fwi_robust.h): the
// elementwise robust source with its sums per trace and its block sums, the small launch that adds the tiles per trace,
// and the radix select behind fwi_residual_median.  Its own object: the other objects keep their pinned kernel counts.
//
// robust_source uses the shared tile of fwi_gather_tile.h (lane = trace, 64 traces by 32 times per block of 256
// threads, 8 consecutive times per thread).  It reads e (and M where W is kept) and writes g (and W): 2 to 4 arrays of
// T per sample, nothing else that grows with nt * ntr.  The kind is a template parameter; within huber the two
// branches are selects.  All arithmetic between the loads and the one rounding of g and W to T is fp64.
//
// The select orders samples by the unsigned bit pattern of |e| in T, which for IEEE numbers with the sign cleared is
// the order of their values, +inf and NaN last.  Most significant digit first, 8 bits a pass (4 passes for fp32, 8 for
// fp64): the histogram of the digit of the keys whose higher digits equal the prefix found so far, then the digit at
// which the running count passes the rank.  Per trace the bins sit in LDS as [digit][lane]: a wave's 64 lanes bump 64
// different addresses (lane and lane + 32 share a bank and are served in different halves), and the waves of a block,
// which walk different times, meet only through the LDS integer atomics, whose result does not depend on their order.
// Every pass reads e again (and M): nt * ntr * passes * (1 or 2) * sizeof(T) bytes.
#include <hip/hip_runtime.h>

#include "fwi_robust.h"
#include "fwi_gather_tile.h"
#include "fwi_kernels.h"

namespace fwi {

namespace {

static_assert(GT_TT == 32, "robust_tiles (fwi_robust.h) counts tiles of 32 times");
constexpr int RB_WAVES = GT_BLOCK / GT_LANES;
constexpr int RB_TBLOCK = 256;

template <typename T, int KIND>
__global__ __launch_bounds__(GT_BLOCK) void robust_source(T *g, T *W, const T *e, const T *m, const double *thresh,
                                                          const double *tw, double *part, int32_t *cnt,
                                                          double *blocksum, int nt, int ntr, int xtiles) {
    __shared__ double sums[RB_WAVES][GT_LANES];  // (GT_BLOCK doubles: the block's tree sum takes them afterwards)
    __shared__ int32_t outs[RB_WAVES][GT_LANES];
    const GatherTile c = gather_tile(xtiles);
    double acc = 0.0, wj = 1.0;
    int32_t beyond = 0;
    if (c.gx < ntr) {
        const double a = thresh[c.gx];
        if (tw) wj = tw[c.gx];
#pragma unroll
        for (int j = 0; j < GT_TO; ++j) {
            if (c.tn0 + j < nt) {
                const int64_t at = (int64_t)(c.tn0 + j) * ntr + c.gx;
                const double ev = (double)e[at], ae = fabs(ev);
                double psi;
                if constexpr (KIND == ROBUST_HUBER) {
                    // (a = +inf: always inside; the other side's inf - inf is computed and not selected)
                    const bool inside = ae <= a;
                    psi = inside ? 1.0 : a / ae;
                    acc = inside ? fma(0.5 * ev, ev, acc) : acc + (a * ae - 0.5 * a * a);
                } else {
                    const double q = ev / a, v = q * q;
                    if constexpr (KIND == ROBUST_HYBRID) {
                        const double s = sqrt(1.0 + v);
                        psi = 1.0 / s;
                        acc += ev * ev / (1.0 + s);
                    } else {
                        psi = 1.0 / (1.0 + v);
                        acc += 0.5 * a * a * log1p(v);
                    }
                }
                beyond += ae > a ? 1 : 0;
                g[at] = (T)(wj * (psi * ev));
                if (W) {
                    const double mv = m ? (double)m[at] : 1.0;
                    W[at] = (T)(wj * (mv * mv) * psi);
                }
            }
        }
    }
    sums[c.grp][c.lane] = acc;
    outs[c.grp][c.lane] = beyond;
    __syncthreads();
    // wave 0 adds the four waves' sums and counts per lane, in wave order
    if (c.grp == 0 && c.gx < ntr) {
        double v = sums[0][c.lane];
        int32_t k = outs[0][c.lane];
#pragma unroll
        for (int q = 1; q < RB_WAVES; ++q) v += sums[q][c.lane], k += outs[q][c.lane];
        const int64_t tile = blockIdx.x / xtiles;
        part[tile * ntr + c.gx] = v;
        cnt[tile * ntr + c.gx] = k;
    }
    __syncthreads();  // the per-lane sums are read: their LDS takes the block's sum
    block_tree_sum_to_partial(wj * acc, &sums[0][0], blocksum);
}

__global__ __launch_bounds__(RB_TBLOCK) void robust_terms(double *jterm, int32_t *nout, const double *part,
                                                          const int32_t *cnt, const double *tw, int tiles, int ntr) {
    const int j = blockIdx.x * RB_TBLOCK + threadIdx.x;
    if (j >= ntr) return;
    double v = 0.0;
    int32_t k = 0;
    for (int64_t t = 0; t < tiles; ++t) v += part[t * ntr + j], k += cnt[t * ntr + j];
    jterm[j] = (tw ? tw[j] : 1.0) * v;
    nout[j] = k;
}

template <typename T> struct Key;
template <> struct Key<float> {
    using U = uint32_t;
    static constexpr int PASSES = 4;
};
template <> struct Key<double> {
    using U = uint64_t;
    static constexpr int PASSES = 8;
};

// the bit pattern of |x|
template <typename T>
__device__ __forceinline__ typename Key<T>::U abs_key(T x) {
    using U = typename Key<T>::U;
    U u;
    __builtin_memcpy(&u, &x, sizeof u);
    return u & ~(U(1) << (8 * sizeof(U) - 1));
}

template <typename T>
__device__ __forceinline__ double key_value(typename Key<T>::U u) {
    T x;
    __builtin_memcpy(&x, &u, sizeof x);
    return (double)x;
}

// bins[0 .. 256) at stride `stride`: the digit at which the running count passes rank r, and the count before it.
// (An empty histogram: digit 0, nothing before it.)
__device__ __forceinline__ void pick_digit(const uint32_t *bins, int stride, uint64_t r, int *digit, uint64_t *before) {
    uint64_t cum = 0;
    bool found = false;
    *digit = 0, *before = 0;
    for (int d = 0; d < 256; ++d) {
        const uint32_t k = bins[d * stride];
        if (!found && cum + k > r) *digit = d, *before = cum, found = true;
        cum += k;
    }
}

template <typename T>
__global__ __launch_bounds__(GT_BLOCK) void median_traces(double *med, int64_t *count, const T *e, const T *m, int nt,
                                                          int ntr) {
    using U = typename Key<T>::U;
    constexpr int PASSES = Key<T>::PASSES;
    __shared__ uint32_t bins[256 * GT_LANES];  // [digit][lane]: 64 KiB
    __shared__ U prefix[GT_LANES];
    __shared__ uint32_t rank[GT_LANES];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int gx = blockIdx.x * GT_LANES + lane;
    const bool live = gx < ntr;
    uint32_t total = 0;  // (of wave 0's lanes: the samples of the trace that count)
    if (grp == 0) prefix[lane] = 0, rank[lane] = 0;
    for (int p = 0; p < PASSES; ++p) {
        const int shift = 8 * (PASSES - 1 - p);
        for (int i = threadIdx.x; i < 256 * GT_LANES; i += GT_BLOCK) bins[i] = 0;
        __syncthreads();
        if (live) {
            const U pre = prefix[lane];
            for (int n = grp; n < nt; n += RB_WAVES) {
                const int64_t at = (int64_t)n * ntr + gx;
                if (m && !(m[at] > T(0))) continue;
                const U key = abs_key<T>(e[at]);
                // the first pass takes every key: there are no higher digits (and no shift by the key's width)
                if (p == 0 || (key >> (shift + 8)) == pre)
                    atomicAdd(&bins[(int)((key >> shift) & 255) * GT_LANES + lane], 1u);
            }
        }
        __syncthreads();
        if (grp == 0 && live) {
            uint64_t r = rank[lane];
            if (p == 0) {
                for (int d = 0; d < 256; ++d) total += bins[d * GT_LANES + lane];
                r = total ? (total - 1) / 2 : 0;
            }
            int digit;
            uint64_t before;
            pick_digit(bins + lane, GT_LANES, r, &digit, &before);
            prefix[lane] = (U)((prefix[lane] << 8) | (U)digit);
            rank[lane] = (uint32_t)(r - before);
        }
        __syncthreads();  // the bins are read before the next pass clears them
    }
    if (grp == 0 && live) {
        med[gx] = total ? key_value<T>(prefix[lane]) : 0.0;
        count[gx] = (int64_t)total;
    }
}

// work: 256 uint32 bins, then the prefix and the rank as uint64
__device__ __forceinline__ uint64_t *median_state(uint32_t *bins) { return (uint64_t *)(bins + 256); }

template <typename T>
__global__ __launch_bounds__(256) void median_hist(uint32_t *bins, const T *e, const T *m, int64_t n, int p) {
    using U = typename Key<T>::U;
    constexpr int PASSES = Key<T>::PASSES;
    __shared__ uint32_t local[256];
    local[threadIdx.x] = 0;
    __syncthreads();
    const U pre = (U)median_state(bins)[0];
    const int shift = 8 * (PASSES - 1 - p);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (m && !(m[i] > T(0))) continue;
        const U key = abs_key<T>(e[i]);
        if (p == 0 || (key >> (shift + 8)) == pre) atomicAdd(&local[(int)((key >> shift) & 255)], 1u);
    }
    __syncthreads();
    const uint32_t k = local[threadIdx.x];
    if (k) atomicAdd(&bins[threadIdx.x], k);
}

template <typename T>
__global__ __launch_bounds__(256) void median_pick(uint32_t *bins, double *med, int64_t *count, int p) {
    using U = typename Key<T>::U;
    uint64_t *state = median_state(bins);
    if (threadIdx.x == 0) {
        uint64_t r = state[1];
        if (p == 0) {
            uint64_t total = 0;
            for (int d = 0; d < 256; ++d) total += bins[d];
            count[0] = (int64_t)total;
            r = total ? (total - 1) / 2 : 0;
        }
        int digit;
        uint64_t before;
        pick_digit(bins, 1, r, &digit, &before);
        const uint64_t pre = (state[0] << 8) | (uint64_t)digit;
        state[0] = pre, state[1] = r - before;
        if (p == Key<T>::PASSES - 1) med[0] = count[0] ? key_value<T>((U)pre) : 0.0;
    }
    __syncthreads();
    bins[threadIdx.x] = 0;  // for the next pass
}

bool robust_shape(int nt, int ntr) { return nt >= 1 && ntr >= 1 && gather_blocks(nt, ntr) <= 0x7fffffff; }

}  // namespace

template <typename T>
hipError_t launch_robust_source(T *g, T *W, const T *e, const T *m, const double *thresh, const double *tw, int kind,
                                double *part, int32_t *cnt, double *blocksum, int nt, int ntr, hipStream_t st) {
    if (!g || !e || !thresh || !part || !cnt || !blocksum || !robust_shape(nt, ntr) || g == m ||
        (W && (W == e || W == m || W == g)))
        return hipErrorInvalidValue;
    const int64_t blocks = gather_blocks(nt, ntr);
    const dim3 grid((unsigned)blocks), block(GT_BLOCK);
    const int xt = gather_xtiles(ntr);
    switch (kind) {
    case ROBUST_HUBER:
        hipLaunchKernelGGL((robust_source<T, ROBUST_HUBER>), grid, block, 0, st, g, W, e, m, thresh, tw, part, cnt,
                           blocksum, nt, ntr, xt);
        break;
    case ROBUST_HYBRID:
        hipLaunchKernelGGL((robust_source<T, ROBUST_HYBRID>), grid, block, 0, st, g, W, e, m, thresh, tw, part, cnt,
                           blocksum, nt, ntr, xt);
        break;
    case ROBUST_CAUCHY:
        hipLaunchKernelGGL((robust_source<T, ROBUST_CAUCHY>), grid, block, 0, st, g, W, e, m, thresh, tw, part, cnt,
                           blocksum, nt, ntr, xt);
        break;
    default:
        return hipErrorInvalidValue;
    }
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    return launch_sum_partials(blocksum, blocks, st);
}

hipError_t launch_robust_terms(double *part, int32_t *cnt, const double *tw, int nt, int ntr, hipStream_t st) {
    if (!part || !cnt || !robust_shape(nt, ntr)) return hipErrorInvalidValue;
    const int tiles = robust_tiles(nt);
    hipLaunchKernelGGL(robust_terms, dim3((unsigned)((ntr + RB_TBLOCK - 1) / RB_TBLOCK)), dim3(RB_TBLOCK), 0, st,
                       part + (size_t)tiles * ntr, cnt + (size_t)tiles * ntr, part, cnt, tw, tiles, ntr);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_median_traces(double *med, int64_t *count, const T *e, const T *m, int nt, int ntr, hipStream_t st) {
    if (!med || !count || !e || !robust_shape(nt, ntr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(median_traces<T>, dim3((unsigned)gather_xtiles(ntr)), dim3(GT_BLOCK), 0, st, med, count, e, m, nt,
                       ntr);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_median_all(double *med, int64_t *count, void *work, const T *e, const T *m, int64_t n, hipStream_t st) {
    if (!med || !count || !work || !e || n < 1 || n > 0xffffffffLL) return hipErrorInvalidValue;
    hipError_t err = hipMemsetAsync(work, 0, median_all_work(), st);
    if (err != hipSuccess) return err;
    uint32_t *bins = (uint32_t *)work;
    // 8 samples or more per thread, at most 1024 blocks: the flush costs 256 global atomics per block
    const int64_t want = (n + 256 * 8 - 1) / (256 * 8);
    const unsigned blocks = (unsigned)(want < 1024 ? want : 1024);
    for (int p = 0; p < Key<T>::PASSES; ++p) {
        hipLaunchKernelGGL(median_hist<T>, dim3(blocks), dim3(256), 0, st, bins, e, m, n, p);
        hipLaunchKernelGGL(median_pick<T>, dim3(1), dim3(256), 0, st, bins, med, count, p);
        if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    return hipSuccess;
}

template hipError_t launch_robust_source<float>(float *, float *, const float *, const float *, const double *,
                                                const double *, int, double *, int32_t *, double *, int, int, hipStream_t);
template hipError_t launch_robust_source<double>(double *, double *, const double *, const double *, const double *,
                                                 const double *, int, double *, int32_t *, double *, int, int,
                                                 hipStream_t);
template hipError_t launch_median_traces<float>(double *, int64_t *, const float *, const float *, int, int, hipStream_t);
template hipError_t launch_median_traces<double>(double *, int64_t *, const double *, const double *, int, int,
                                                 hipStream_t);
template hipError_t launch_median_all<float>(double *, int64_t *, void *, const float *, const float *, int64_t,
                                             hipStream_t);
template hipError_t launch_median_all<double>(double *, int64_t *, void *, const double *, const double *, int64_t,
                                              hipStream_t);

}  // namespace fwi
