// Normal equations and application of a short two-sided matching filter along time on (nt, ntr) trace gathers
// (fwi_match.h).  Its own object: every other object keeps its pinned kernel count.
//
// match_normal.  With a = k + L and z_n[a] = s[n + L - a] the matrix is G[a, b] = sum_{n, j} M^2[n, j] z_n[a] z_n[b]: a
// small SYRK over shifted copies of one gather, K^2 / 2 fp64 FMAs per sample.  Lane = trace; a wave owns one 8 x 8
// tile (ta, tb), ta <= tb, of G in 64 accumulators per lane and walks time in steps of 8: the 15 rows of s that 8 times
// and 8 shifts can pair are kept in registers per tile side, as a window that moves by 8 rows per step through
// compile-time indices (a run-time-indexed local array would go to scratch), so a step costs 16 new loads (24 on a
// diagonal tile, which also carries b) for 512 FMAs.  The rows are read from global memory: every wave of a trace tile
// reads the same few rows, which the caches hold, while the K + 63 rows by 64 traces a block would stage exceed 64 KB of
// LDS in fp64 at L = 64.  The gather is cut into units of 64 traces x 64 times; slice s of at most 256 takes the units
// s, s + slices, ... in ascending order, and the wave of (slice, tile) sums them into the same accumulators, folds its 64
// lanes by a fixed exchange tree that leaves entry l of the tile on lane l, and stores the tile into its slice of
// `partial`.  match_reduce adds the slices in ascending order and writes G (both triangles) and b.  The last tile row and
// column also form the shifts a >= K up to the tile edge; those entries are never read again.
//
// match_apply.  The tile and the fixed-order sum of squares are the shared ones of fwi_gather_tile.h, not its march:
// K <= 129, so nothing is chunked.  The coefficients sit in LDS (padded to a multiple of 8; the padding is skipped, not
// multiplied), the 15 input rows that 8 outputs and 8 coefficients can pair in a register window that is read from
// global memory.  Sums over ascending k, in fp64.
//
// No atomics anywhere.
#include <hip/hip_runtime.h>

#include "fwi_gather_tile.h"
#include "fwi_kernels.h"
#include "fwi_match.h"

namespace fwi {

namespace {

constexpr int MT = GT_TO;         // tile edge of match_normal, outputs per thread of match_apply
constexpr int MN_TT = 64;         // times per unit of match_normal
constexpr int MN_SLICES = 256;    // most slices of the partials buffer
constexpr int MATCH_KP = (2 * MATCH_LMAX + 1 + MT - 1) / MT * MT;  // 136
static_assert(MN_TT % MT == 0, "whole steps of 8");

struct NormalArgs {
    int nt, ntr, L, nT, P, xtiles, units, slices;
    int64_t slice_len;  // 64 P + 8 nT
};

NormalArgs normal_plan(int nt, int ntr, int L) {
    NormalArgs a;
    a.nt = nt, a.ntr = ntr, a.L = L;
    a.nT = (2 * L + 1 + MT - 1) / MT;
    a.P = a.nT * (a.nT + 1) / 2;
    a.xtiles = (ntr + 63) / 64;
    const int64_t units = (int64_t)a.xtiles * ((nt + MN_TT - 1) / MN_TT);
    a.units = units > 0x7fffffff ? 0 : (int)units;
    a.slices = a.units < MN_SLICES ? a.units : MN_SLICES;
    a.slice_len = (int64_t)MT * MT * a.P + (int64_t)MT * a.nT;
    return a;
}

// One exchange step of the wave's sum: the lanes whose bit H is set keep entries i + H, the others entries i, each
// adding its partner's share.  After the steps 32, 16, .., 1 lane l holds the wave's total of entry l.
#define MATCH_FOLD(v, H)                                           \
    _Pragma("unroll") for (int i_ = 0; i_ < (H); ++i_) {           \
        const bool up_ = (lane & (H)) != 0;                        \
        const double send_ = up_ ? v[i_] : v[i_ + (H)];            \
        const double keep_ = up_ ? v[i_ + (H)] : v[i_];            \
        v[i_] = keep_ + __shfl_xor(send_, (H));                    \
    }

template <typename T>
__global__ __launch_bounds__(64) void match_normal(const T *__restrict__ s, const T *__restrict__ d,
                                                   const T *__restrict__ w, NormalArgs a, double *__restrict__ partial) {
    const int lane = threadIdx.x;
    const int slice = (int)(blockIdx.x / (unsigned)a.P), p = (int)(blockIdx.x % (unsigned)a.P);
    int ta = 0, rem = p;  // tile pairs in row-major order over the upper triangle
    while (rem >= a.nT - ta) {
        rem -= a.nT - ta;
        ++ta;
    }
    const int tb = ta + rem;
    const bool diag = ta == tb;
    const int nt = a.nt, ntr = a.ntr;

    double acc[MT * MT], bacc[MT];
#pragma unroll
    for (int i = 0; i < MT * MT; ++i) acc[i] = 0.0;
#pragma unroll
    for (int i = 0; i < MT; ++i) bacc[i] = 0.0;

    for (int u = slice; u < a.units; u += a.slices) {
        const int gx = (u % a.xtiles) * 64 + lane, t0 = (u / a.xtiles) * MN_TT;
        const int t1 = t0 + MN_TT < nt ? t0 + MN_TT : nt;
        const bool live = gx < ntr;
        auto S = [&](int row) -> double {
            return (row >= 0 && row < nt && live) ? (double)s[(int64_t)row * ntr + gx] : 0.0;
        };
        // wa[q] = s[ra + q], ra = n0 + L - 8 ta - 7: time n0 + i meets shift a = 8 ta + a' in wa[i + 7 - a']
        int ra = t0 + a.L - MT * ta - (MT - 1), rb = t0 + a.L - MT * tb - (MT - 1);
        double wa[2 * MT - 1], wb[2 * MT - 1];
#pragma unroll
        for (int q = 0; q < MT - 1; ++q) {
            wa[q + MT] = S(ra + q);
            wb[q + MT] = S(rb + q);
        }
#pragma unroll 1
        for (int n0 = t0; n0 < t1; n0 += MT, ra += MT, rb += MT) {
#pragma unroll
            for (int q = 0; q < MT - 1; ++q) {
                wa[q] = wa[q + MT];
                wb[q] = wb[q + MT];
            }
#pragma unroll
            for (int q = MT - 1; q < 2 * MT - 1; ++q) {
                wa[q] = S(ra + q);
                wb[q] = S(rb + q);
            }
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int n = n0 + i;
                const bool in = n < t1 && live;  // (times of the next unit carry no weight here)
                const int64_t at = (int64_t)n * ntr + gx;
                const double wv = !in ? 0.0 : w ? (double)w[at] : 1.0;
                const double m = wv * wv;
#pragma unroll
                for (int aa = 0; aa < MT; ++aa) {
                    const double t = m * wa[i + MT - 1 - aa];
#pragma unroll
                    for (int bb = 0; bb < MT; ++bb) acc[aa * MT + bb] = fma(t, wb[i + MT - 1 - bb], acc[aa * MT + bb]);
                }
                if (diag) {
                    const double md = in ? m * (double)d[at] : 0.0;
#pragma unroll
                    for (int aa = 0; aa < MT; ++aa) bacc[aa] = fma(md, wa[i + MT - 1 - aa], bacc[aa]);
                }
            }
        }
    }

    MATCH_FOLD(acc, 32)
    MATCH_FOLD(acc, 16)
    MATCH_FOLD(acc, 8)
    MATCH_FOLD(acc, 4)
    MATCH_FOLD(acc, 2)
    MATCH_FOLD(acc, 1)
    double *out = partial + (int64_t)slice * a.slice_len;
    out[(int64_t)p * (MT * MT) + lane] = acc[0];
    if (diag) {
        MATCH_FOLD(bacc, 4)
        MATCH_FOLD(bacc, 2)
        MATCH_FOLD(bacc, 1)
        double v = bacc[0];  // the total of entry lane & 7 over this group of 8 lanes
        v += __shfl_xor(v, 8);
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (lane < MT) out[(int64_t)a.P * (MT * MT) + ta * MT + lane] = v;
    }
}

#undef MATCH_FOLD

// normal := the sum of the slices in ascending order: G in full (entry (a, b) and (b, a) read the same sums), then b
__global__ __launch_bounds__(256) void match_reduce(const double *__restrict__ partial, double *__restrict__ normal,
                                                    NormalArgs a) {
    const int K = 2 * a.L + 1;
    const int idx = (int)(blockIdx.x * 256 + threadIdx.x);
    if (idx >= K * K + K) return;
    int64_t off;
    if (idx < K * K) {
        int r = idx / K, c = idx % K;
        if (r > c) {
            const int t = r;
            r = c, c = t;
        }
        const int ta = r / MT, tb = c / MT;
        const int p = ta * a.nT - ta * (ta - 1) / 2 + (tb - ta);
        off = (int64_t)p * (MT * MT) + (r % MT) * MT + (c % MT);
    } else {
        off = (int64_t)a.P * (MT * MT) + (idx - K * K);
    }
    double sum = 0.0;
    for (int sl = 0; sl < a.slices; ++sl) sum += partial[(int64_t)sl * a.slice_len + off];
    normal[idx] = sum;
}

struct ApplyArgs {
    int nt, ntr, L, xtiles;
};

template <typename T, bool CORR>
__global__ __launch_bounds__(GT_BLOCK) void match_apply(T *__restrict__ out, const T *__restrict__ in,
                                                        const T *__restrict__ sub, const T *__restrict__ wpre,
                                                        const T *__restrict__ wpost, const double *__restrict__ f,
                                                        ApplyArgs a, double *__restrict__ partial) {
    __shared__ double sF[MATCH_KP];
    __shared__ double sRed[GT_BLOCK];
    const GatherTile c = gather_tile(a.xtiles);
    const int tid = threadIdx.x, gx = c.gx, tn0 = c.tn0;
    const int nt = a.nt, ntr = a.ntr, K = 2 * a.L + 1, Kp = (K + MT - 1) / MT * MT;
    for (int k = tid; k < Kp; k += GT_BLOCK) sF[k] = k < K ? f[k] : 0.0;
    __syncthreads();
    const bool live = gx < ntr;
    auto X = [&](int row) -> double {
        if (!(row >= 0 && row < nt && live)) return 0.0;
        const int64_t at = (int64_t)row * ntr + gx;
        const double v = (double)in[at];
        return wpre ? v * (double)wpre[at] : v;
    };
    double acc[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[j] = 0.0;
    // coefficient kb + i is f_k, k = kb + i - L.  Convolution: output j reads row tn0 + j - k = base + (j - i + 7),
    // base = tn0 + L - kb - 7, which falls by 8 per group; correlation: row tn0 + j + k = base + (j + i),
    // base = tn0 - L + kb, which rises by 8.
    double x[2 * MT - 1];
    int base = CORR ? tn0 - a.L : tn0 + a.L - (MT - 1);
#pragma unroll
    for (int q = 0; q < MT - 1; ++q) {
        if (CORR)
            x[q + MT] = X(base + q);
        else
            x[q] = X(base + MT + q);
    }
#pragma unroll 1
    for (int kb = 0; kb < Kp; kb += MT, base += CORR ? MT : -MT) {
        if (CORR) {
#pragma unroll
            for (int q = 0; q < MT - 1; ++q) x[q] = x[q + MT];
#pragma unroll
            for (int q = MT - 1; q < 2 * MT - 1; ++q) x[q] = X(base + q);
        } else {
#pragma unroll
            for (int q = 2 * MT - 2; q >= MT; --q) x[q] = x[q - MT];
#pragma unroll
            for (int q = 0; q < MT; ++q) x[q] = X(base + q);
        }
        double c[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) c[i] = sF[kb + i];
        if (kb + MT <= K) {
#pragma unroll
            for (int i = 0; i < MT; ++i) {
#pragma unroll
                for (int j = 0; j < MT; ++j) acc[j] = fma(c[i], x[CORR ? j + i : j - i + MT - 1], acc[j]);
            }
        } else {  // the last group: the coefficients past f_L do not exist, so their rows (finite or not) add nothing
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                if (kb + i < K) {
#pragma unroll
                    for (int j = 0; j < MT; ++j) acc[j] = fma(c[i], x[CORR ? j + i : j - i + MT - 1], acc[j]);
                }
            }
        }
    }

    double sq = 0.0;
    if (live) {
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            if (tn0 + j < nt) {
                const int64_t at = (int64_t)(tn0 + j) * ntr + gx;
                double v = acc[j];
                if (sub) v -= (double)sub[at];
                if (wpost) v *= (double)wpost[at];
                out[at] = (T)v;
                sq += v * v;
            }
        }
    }
    if (partial) block_tree_sum_to_partial(sq, sRed, partial);
}

}  // namespace

int64_t match_normal_partials(int nt, int ntr, int L) {
    const NormalArgs a = normal_plan(nt, ntr, L);
    return (int64_t)a.slices * a.slice_len;
}

template <typename T>
hipError_t launch_match_normal(double *normal, double *partial, const T *s, const T *d, const T *w, int L, int nt,
                               int ntr, hipStream_t st) {
    if (!normal || !partial || !s || !d || nt < 1 || ntr < 1 || L < 0 || L > MATCH_LMAX) return hipErrorInvalidValue;
    const NormalArgs a = normal_plan(nt, ntr, L);
    if (a.units < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(match_normal<T>, dim3((unsigned)(a.slices * a.P)), dim3(64), 0, st, s, d, w, a, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int K = 2 * L + 1;
    hipLaunchKernelGGL(match_reduce, dim3((unsigned)((K * K + K + 255) / 256)), dim3(256), 0, st,
                       (const double *)partial, normal, a);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_match_apply(T *out, const T *in, const T *sub, const T *wpre, const T *wpost, const double *f, int L,
                              bool corr, int nt, int ntr, double *partial, hipStream_t st) {
    const int64_t blocks = gather_blocks(nt, ntr);
    if (!out || !in || !f || nt < 1 || ntr < 1 || L < 0 || L > MATCH_LMAX || blocks > 0x7fffffff || out == in ||
        out == sub || out == wpre || out == wpost)
        return hipErrorInvalidValue;
    ApplyArgs a;
    a.nt = nt, a.ntr = ntr, a.L = L, a.xtiles = gather_xtiles(ntr);
    if (corr)
        hipLaunchKernelGGL((match_apply<T, true>), dim3((unsigned)blocks), dim3(GT_BLOCK), 0, st, out, in, sub, wpre,
                           wpost, f, a, partial);
    else
        hipLaunchKernelGGL((match_apply<T, false>), dim3((unsigned)blocks), dim3(GT_BLOCK), 0, st, out, in, sub, wpre,
                           wpost, f, a, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !partial) return e;
    return launch_sum_partials(partial, blocks, st);
}

template hipError_t launch_match_normal<float>(double *, double *, const float *, const float *, const float *, int, int,
                                               int, hipStream_t);
template hipError_t launch_match_normal<double>(double *, double *, const double *, const double *, const double *, int,
                                                int, int, hipStream_t);
template hipError_t launch_match_apply<float>(float *, const float *, const float *, const float *, const float *,
                                              const double *, int, bool, int, int, double *, hipStream_t);
template hipError_t launch_match_apply<double>(double *, const double *, const double *, const double *, const double *,
                                               const double *, int, bool, int, int, double *, hipStream_t);

}  // namespace fwi
