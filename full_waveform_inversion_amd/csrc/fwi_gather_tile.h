// What the kernels that filter (nt, ntr) trace gathers along time share (fwi_data.hip, fwi_envelope.hip, fwi_match.hip):
// the tile, the block's fixed-order sum (fwi_reg.hip takes that too) and the march of a FIR filter's input rows through
// LDS.  Time is the slow axis of a gather, the trace index the fast one.
//
// Tile.  Lane = trace: every global load and store runs along the fast axis.  A block of GT_BLOCK = 256 threads owns
// GT_LANES = 64 traces by GT_TT = 32 output times; each of its four waves keeps GT_TO = 8 consecutive output times per
// lane in registers.  Block b owns the trace tile b % xtiles and the time tile b / xtiles.
//
// Sums.  A thread sums its own terms over ascending time, block_tree_sum_to_partial adds the block's 256 values by a
// fixed halving tree into partial[block], and launch_sum_partials (fwi_kernels.h) adds the partials in a fixed order:
// no atomics, equal inputs give equal bits.
//
// March (gather_march).  out[n] = sum_kappa w(kappa) x[n + kappa], kappa = row - output, |kappa| <= reach.  The taps sit
// in LDS behind the rows.  The input rows t0 - reach .. t0 + GT_TT + reach - 1 that the tile needs do not fit LDS at the
// reach of a real band-pass, so they pass through it in chunks of CH rows, in ascending time, the NS signals of a kernel
// together: per chunk
//   stage   the chunk's rows as fp64, as the kernel's staging functor gives them; rows outside [0, nt) and traces >= ntr
//           are not read, their slots hold zeros;
//   sum     per 8 rows: the 15 weights w(kappa) that 8 rows and 8 outputs can pair (zero where the filter has none) go to
//           registers, then every row's x is read once from LDS (lane-contiguous doubles: no bank conflict) and added
//           into the 8 accumulators of each signal: 64 fp64 FMAs per signal for 15 + 8 LDS reads.  A group of rows none
//           of which the wave's outputs can reach is skipped (the test is the same for a whole wave).
// For every output the terms are added by fma over ascending row time, in fp64; rounding to T is the caller's, once, at
// its store.  Everything is indexed at compile time and inlined: accumulators and weights stay in registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fwi {

constexpr int GT_LANES = 64, GT_TO = 8, GT_TT = 4 * GT_TO, GT_BLOCK = 256;
static_assert(GT_BLOCK == 64 * (GT_TT / GT_TO) && GT_LANES == 64, "one wave per GT_TO output times");

inline int gather_xtiles(int ntr) { return (ntr + GT_LANES - 1) / GT_LANES; }

// number of blocks of one launch over (nt, ntr) = number of its partial sums; a buffer handed over as `partial` holds
// one double more (the total)
inline int64_t gather_blocks(int nt, int ntr) { return (int64_t)gather_xtiles(ntr) * ((nt + GT_TT - 1) / GT_TT); }

struct GatherTile {
    int x0, t0;      // the tile's first trace and first output time
    int lane, grp;   // this thread's lane and its wave within the block
    int gx, tn0;     // this thread's trace and its first output time
};

__device__ __forceinline__ GatherTile gather_tile(int xtiles) {
    GatherTile c;
    c.lane = threadIdx.x & 63, c.grp = threadIdx.x >> 6;
    c.x0 = (int)(blockIdx.x % xtiles) * GT_LANES, c.t0 = (int)(blockIdx.x / xtiles) * GT_TT;
    c.gx = c.x0 + c.lane, c.tn0 = c.t0 + c.grp * GT_TO;
    return c;
}

// partial[block] := the sum of the block's 256 values v, by a halving tree over lds[0 .. 256).  The LDS is the caller's:
// where it held something else, the caller's barrier precedes the call.
__device__ __forceinline__ void block_tree_sum_to_partial(double v, double *lds, double *partial) {
    const int tid = threadIdx.x;
    lds[tid] = v;
    __syncthreads();
    for (int s = GT_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) lds[tid] += lds[tid + s];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = lds[0];
}

// Weight policies: w(kappa) from the taps in LDS.  PARITY: the policy can leave out the products of even kappa.
struct SymmetricTaps {  // w(kappa) = b_|kappa|, |kappa| <= reach; b: b_0 .. b_reach
    static constexpr bool PARITY = false;
    const double *b;
    int reach;
    __device__ __forceinline__ double operator()(int k) const {
        const int kk = k < 0 ? -k : k;
        return kk <= reach ? b[kk] : 0.0;
    }
};

// A Hilbert transformer's even taps are zero.  Where the caller says so (odd_only), a group forms only the products
// whose kappa is odd: which those are depends on the parity of the group's first kappa alone, which is the same for a
// whole wave, so the branch is uniform and each side is straight-line code of half the FMAs.  The products left out are
// 0 * x, which add nothing to a finite sum: the bits do not depend on it.
struct AntisymmetricTaps {  // w(kappa) = -sign(kappa) h_|kappa|, 1 <= |kappa| <= reach; h: h_1 .. h_reach
    static constexpr bool PARITY = true;
    const double *h;
    int reach;
    bool odd_only;
    __device__ __forceinline__ double operator()(int k) const {
        const int kk = k < 0 ? -k : k;
        const double hv = (kk >= 1 && kk <= reach) ? h[kk - 1] : 0.0;
        return k < 0 ? hv : -hv;  // x[n - k] enters with +h_k, x[n + k] with -h_k
    }
};

// one group of GT_TO rows (row points at the first one's slot of this lane, the signals CH rows apart) against the
// thread's GT_TO outputs; d0 = kappa of (row 0, output 0): the group pairs kappa in d0 - 7 .. d0 + 7.  PAR < 0: every
// product; otherwise PAR = d0 & 1 and only the products with odd kappa = d0 + i - j.
template <int NS, int CH, int PAR, typename Weight>
__device__ __forceinline__ void gather_group(double (&acc)[NS][GT_TO], const double *row, const Weight &wt, int d0) {
    double w[2 * GT_TO - 1];
#pragma unroll
    for (int q = 0; q < 2 * GT_TO - 1; ++q) {
        if (PAR >= 0 && ((PAR + q) & 1)) continue;  // kappa = d0 + q - 7 is even
        w[q] = wt(d0 + q - (GT_TO - 1));
    }
#pragma unroll
    for (int i = 0; i < GT_TO; ++i) {
        double xv[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) xv[s] = row[(s * CH + i) * GT_LANES];
#pragma unroll
        for (int j = 0; j < GT_TO; ++j) {
            const int q = i - j + GT_TO - 1;
            if (PAR >= 0 && ((PAR + q) & 1)) continue;
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s][j] = fma(w[q], xv[s], acc[s][j]);
        }
    }
}

// acc[s][j] := sum_kappa w(kappa) x_s[tn0 + j + kappa, gx] for the NS signals; sX: NS * CH * GT_LANES doubles of LDS.
// stage(s, at): the fp64 value of signal s at the flat index at = row * ntr + trace of a sample inside the gather.
// The taps that wt reads are in LDS before the first chunk's barrier.
template <int NS, int CH, typename Stage, typename Weight>
__device__ __forceinline__ void gather_march(double (&acc)[NS][GT_TO], double *sX, const GatherTile &c, int nt, int ntr,
                                             Stage stage, Weight wt) {
    static_assert(CH % GT_TO == 0 && CH * GT_LANES >= GT_BLOCK, "whole groups of rows; room for the block's sum");
    const int tid = threadIdx.x, reach = wt.reach;
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int j = 0; j < GT_TO; ++j) acc[s][j] = 0.0;

    const int lo = c.t0 - reach > 0 ? c.t0 - reach : 0, hi = c.t0 + GT_TT + reach < nt ? c.t0 + GT_TT + reach : nt;
    for (int m0 = lo; m0 < hi; m0 += CH) {
        __syncthreads();  // the chunk before is used up
        for (int i = tid; i < CH * GT_LANES; i += GT_BLOCK) {
            const int gm = m0 + (i >> 6), g = c.x0 + (i & 63);
            double v[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) v[s] = 0.0;
            if (gm < hi && g < ntr) {
                const int64_t at = (int64_t)gm * ntr + g;
#pragma unroll
                for (int s = 0; s < NS; ++s) v[s] = stage(s, at);
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) sX[s * CH * GT_LANES + i] = v[s];
        }
        __syncthreads();
#pragma unroll 1
        for (int mb = 0; mb < CH; mb += GT_TO) {
            const int d0 = m0 + mb - c.tn0;
            if (m0 + mb >= hi || d0 + (GT_TO - 1) < -reach || d0 - (GT_TO - 1) > reach) continue;
            const double *row = sX + mb * GT_LANES + c.lane;
            if constexpr (Weight::PARITY) {
                if (!wt.odd_only)
                    gather_group<NS, CH, -1>(acc, row, wt, d0);
                else if (d0 & 1)
                    gather_group<NS, CH, 1>(acc, row, wt, d0);
                else
                    gather_group<NS, CH, 0>(acc, row, wt, d0);
            } else {
                gather_group<NS, CH, -1>(acc, row, wt, d0);
            }
        }
    }
}

}  // namespace fwi
