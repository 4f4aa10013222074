// Device functions shared by the eikonal kernels (fwi_eikonal.hip), the tangent kernels (fwi_eikonal_tangent.hip) and the
// stage kernels (fwi_eikonal_stage.hip): the tile geometry, THE local solver, the weights derived from it and the bodies
// of the forward and the tangent sweep.  Every kernel of the three units takes G, "T_i < G_i" and the upwind choice from
// here, so the units cannot disagree on a decision of the arithmetic.  At the end, the two host helpers that size the
// launches of all units (blocks256, eik_grid).  Not a header for other code:
// include it inside namespace fwi { namespace { ... } }, after fwi_eikonal.h and <math.h>.
#pragma once

template <int ND>
struct Eik {
    static constexpr int TL = ND == 2 ? EIK_TILE2 : EIK_TILE3;           // tile edge
    static constexpr int NT = ND == 2 ? TL * TL : TL * TL * TL;           // threads = cells of a tile
};

template <typename T>
__device__ __forceinline__ T eik_inf() {
    return (T)INFINITY;
}
template <typename T>
__device__ __forceinline__ T eik_min(T x, T y) {
    return x < y ? x : y;
}
template <typename T>
__device__ __forceinline__ T eik_max(T x, T y) {
    return x < y ? y : x;
}
// correctly rounded, as the twin's (the compiler's default for the plain functions; the _rn intrinsic of fp32 is the
// native approximation)
__device__ __forceinline__ float eik_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double eik_sqrt(double x) { return sqrt(x); }

// extents and compact strides per axis, grid order (z, [y,] x)
template <int ND>
__device__ __forceinline__ void eik_dims(const GridDesc &g, int (&n)[ND], int64_t (&st)[ND]) {
    if (ND == 2) {
        n[0] = g.nz, n[ND - 1] = g.nx;
        st[0] = g.cx, st[ND - 1] = 1;
    } else {
        n[0] = g.nz, n[1] = g.ny, n[ND - 1] = g.nx;
        st[0] = (int64_t)g.ny * g.cx, st[1] = g.cx, st[ND - 1] = 1;
    }
}
// first cell of this workgroup's tile
template <int ND>
__device__ __forceinline__ void eik_origin(int (&o)[ND]) {
    constexpr int TL = Eik<ND>::TL;
    if (ND == 2) {
        o[0] = blockIdx.y * TL, o[ND - 1] = blockIdx.x * TL;
    } else {
        o[0] = blockIdx.z * TL, o[1] = blockIdx.y * TL, o[ND - 1] = blockIdx.x * TL;
    }
}
// cell i of a box of edge P, first axis slowest
template <int ND>
__device__ __forceinline__ void eik_decode(int i, int P, int (&l)[ND]) {
    if (ND == 2) {
        l[0] = i / P, l[ND - 1] = i % P;
    } else {
        l[0] = i / (P * P), l[1] = (i / P) % P, l[ND - 1] = i % P;
    }
}
// the grid cell at o + l - halo: whether it exists, and its compact index
template <int ND>
__device__ __forceinline__ bool eik_cell(const int (&n)[ND], const int64_t (&st)[ND], const int (&o)[ND],
                                         const int (&l)[ND], int halo, int64_t &gi) {
    bool ok = true;
    gi = 0;
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const int p = o[d] + l[d] - halo;
        ok = ok && p >= 0 && p < n[d];
        gi += (int64_t)p * st[d];
    }
    return ok;
}

// THE local solver: every kernel here gets G (and with it "T_i < G_i") from this one function.  No contraction: the
// operations are the twin's, one rounding each.
template <typename T, int ND>
__device__ __forceinline__ T eik_local(const T (&t)[ND], T f) {
#pragma clang fp contract(off)
    T a, b, c;
    if (ND == 2) {
        a = eik_min(t[0], t[ND - 1]), b = eik_max(t[0], t[ND - 1]), c = eik_inf<T>();
    } else {
        const T lo = eik_min(t[0], t[1]), hi = eik_max(t[0], t[1]);
        a = eik_min(lo, t[ND - 1]);
        c = eik_max(hi, t[ND - 1]);
        b = eik_max(lo, eik_min(hi, t[ND - 1]));
    }
    const T x1 = a + f;
    if (x1 <= b) return x1;
    const T bp = b - a;
    const T x2 = a + (bp + eik_sqrt((T)2 * f * f - bp * bp)) / (T)2;
    if (x2 <= c) return x2;
    const T cp = c - a;
    const T S = bp + cp, Q = bp * bp + cp * cp;
    return a + (S + eik_sqrt(S * S - (T)3 * (Q - f * f))) / (T)3;
}

// dG/dt_d per axis (0 on inactive axes, where T_i < G_i and where T_i = inf) and den = sum over the active axes of
// T_i - t_d (0 likewise); live: T_i is finite and not below G_i (the cell is determined by its neighbours)
template <typename T, int ND>
__device__ __forceinline__ void eik_weights(T Ti, const T (&t)[ND], T f, T (&w)[ND], T &den, bool &live) {
#pragma clang fp contract(off)
    const T G = eik_local<T, ND>(t, f);
    live = Ti < eik_inf<T>() && !(Ti < G);
    T diff[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) diff[d] = (live && t[d] < Ti) ? Ti - t[d] : (T)0;
    den = diff[0];
#pragma unroll
    for (int d = 1; d < ND; ++d) den = den + diff[d];
#pragma unroll
    for (int d = 0; d < ND; ++d) w[d] = den > (T)0 ? diff[d] / den : (T)0;
}
template <typename T, int ND>
__device__ __forceinline__ void eik_weights(T Ti, const T (&t)[ND], T f, T (&w)[ND], T &den) {
    bool live;
    eik_weights<T, ND>(Ti, t, f, w, den, live);
}

// upwind times of the grid cell at position p from a compact array in memory; lower[d]: the upwind neighbour is the
// lower-index one (ties: yes)
template <typename T, int ND>
__device__ __forceinline__ void eik_fetch(const T *t, const int (&n)[ND], const int64_t (&st)[ND], const int (&p)[ND],
                                          int64_t gi, T (&tt)[ND], bool (&lower)[ND]) {
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const T lo = p[d] > 0 ? t[gi - st[d]] : eik_inf<T>();
        const T hi = p[d] < n[d] - 1 ? t[gi + st[d]] : eik_inf<T>();
        tt[d] = eik_min(lo, hi);
        lower[d] = lo <= hi;
    }
}

// a model-space value as a slowness perturbation: the transposes of g_c = -g_s / c^2 and g_m = g_s c / 2
template <typename T>
__device__ __forceinline__ T eik_dslowness(T dm, T cv, int wrt_velocity) {
#pragma clang fp contract(off)
    return wrt_velocity ? -dm / (cv * cv) : dm * cv / (T)2;
}

// One launch of the block-Jacobi forward sweep for this workgroup's tile: K inner sweeps of min(T, G) with one frozen
// cell around the tile, the interior written to `out`, *flag raised when an interior cell changed.  WALL: a cell with
// wall != 0 is never updated (it holds +inf in both slots, so to its neighbours it is a cell outside the grid); without
// WALL the pointer is not read.  The body of eikonal_sweep (fwi_eikonal.hip) and of eikonal_stage_sweep
// (fwi_eikonal_stage.hip).
template <typename T, int ND, bool WALL>
__device__ __forceinline__ void eik_sweep_tile(const GridDesc &g, const T *__restrict__ in, T *__restrict__ out,
                                               const T *__restrict__ c, const T *__restrict__ wall, T h, int K,
                                               int *flag) {
#pragma clang fp contract(off)
    constexpr int TL = Eik<ND>::TL, NT = Eik<ND>::NT, P = TL + 2;
    constexpr int NP = ND == 2 ? P * P : P * P * P;
    __shared__ T sT[NP];
    int n[ND], o[ND], l[ND];
    int64_t st[ND], gi;
    eik_dims<ND>(g, n, st);
    eik_origin<ND>(o);
    for (int i = threadIdx.x; i < NP; i += NT) {  // the tile and one frozen cell around it; +inf outside the grid
        eik_decode<ND>(i, P, l);
        sT[i] = eik_cell<ND>(n, st, o, l, 1, gi) ? in[gi] : eik_inf<T>();
    }
    eik_decode<ND>(threadIdx.x, TL, l);
    const bool valid = eik_cell<ND>(n, st, o, l, 0, gi);
    int li = 0, ls[ND];  // this thread's cell in the LDS box, and the box's strides
    {
        int s = 1;
        for (int d = ND - 1; d >= 0; --d) {
            ls[d] = s;
            li += (l[d] + 1) * s;
            s *= P;
        }
    }
    const T f = valid ? ((T)1 / c[gi]) * h : (T)1;
    const bool open = valid && !(WALL && wall[gi] != (T)0);  // a walled cell is never updated
    __syncthreads();
    const T orig = sT[li];
    T cur = orig;
    for (int k = 0; k < K; ++k) {
        T t[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) t[d] = eik_min(sT[li - ls[d]], sT[li + ls[d]]);
        const T nw = open ? eik_min(cur, eik_local<T, ND>(t, f)) : cur;
        __syncthreads();
        sT[li] = nw;
        cur = nw;
        __syncthreads();
    }
    if (valid) out[gi] = cur;
    if (__syncthreads_or(valid && cur != orig) && threadIdx.x == 0) atomicMax(flag, 1);
}

// One launch of the block-Jacobi tangent sweep for this workgroup's tile: K inner sweeps of x <- b + A x on its live
// cells, with b_i formed from dm_i and c_i (B0: plus b0_i; without B0 the pointer is not read).  A cell that is not
// live stays as it is.  The body of eikonal_tangent_sweep (fwi_eikonal_tangent.hip) and of eikonal_stage_tangent_sweep
// (fwi_eikonal_stage.hip).
template <typename T, int ND, bool B0>
__device__ __forceinline__ void eik_tangent_tile(const GridDesc &g, const T *__restrict__ tim, const T *__restrict__ dm,
                                                 const T *__restrict__ b0, const T *__restrict__ in,
                                                 T *__restrict__ out, const T *__restrict__ c, T h, int wrt_velocity,
                                                 int K, int *flag) {
#pragma clang fp contract(off)
    constexpr int TL = Eik<ND>::TL, NT = Eik<ND>::NT, P = TL + 2;
    constexpr int NP = ND == 2 ? P * P : P * P * P;
    __shared__ T sT[NP];  // times, one cell around the tile (+inf outside the grid)
    __shared__ T sX[NP];  // the iterate, one frozen cell around the tile (0 outside the grid)
    int n[ND], o[ND], l[ND];
    int64_t st[ND], gi;
    eik_dims<ND>(g, n, st);
    eik_origin<ND>(o);
    for (int i = threadIdx.x; i < NP; i += NT) {
        eik_decode<ND>(i, P, l);
        const bool ok = eik_cell<ND>(n, st, o, l, 1, gi);
        sT[i] = ok ? tim[gi] : eik_inf<T>();
        sX[i] = ok ? in[gi] : (T)0;
    }
    eik_decode<ND>(threadIdx.x, TL, l);
    const bool valid = eik_cell<ND>(n, st, o, l, 0, gi);
    int li = 0, ls[ND];  // this thread's cell in the LDS boxes, and their strides
    {
        int s = 1;
        for (int d = ND - 1; d >= 0; --d) {
            ls[d] = s;
            li += (l[d] + 1) * s;
            s *= P;
        }
    }
    __syncthreads();
    // the local solver once per tile cell: the weights of this cell's own upwind neighbours and its right-hand side
    T w[ND], b = (T)0;
    int nb[ND];
    bool live = false;
#pragma unroll
    for (int d = 0; d < ND; ++d) w[d] = (T)0, nb[d] = li;
    if (valid) {
        T t[ND], den;
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const T lo = sT[li - ls[d]], hi = sT[li + ls[d]];
            t[d] = eik_min(lo, hi);
            nb[d] = lo <= hi ? li - ls[d] : li + ls[d];
        }
        const T cv = c[gi], s = (T)1 / cv;
        eik_weights<T, ND>(sT[li], t, s * h, w, den, live);
        const T dGds = den > (T)0 ? s * h * h / den : (T)0;
        b = dGds * eik_dslowness<T>(dm[gi], cv, wrt_velocity);
        if (B0) b = b + b0[gi];  // after b_i, before the axis terms
    }
    const T orig = sX[li];
    T cur = orig;
    for (int k = 0; k < K; ++k) {
        T acc = b;  // gather form: this cell's own upwind neighbours, axis by axis after b
#pragma unroll
        for (int d = 0; d < ND; ++d) acc = acc + w[d] * sX[nb[d]];
        __syncthreads();
        if (live) sX[li] = acc, cur = acc;  // a cell that is not live stays as the init launches left it
        __syncthreads();
    }
    if (valid) out[gi] = cur;
    if (__syncthreads_or(valid && cur != orig) && threadIdx.x == 0) atomicMax(flag, 1);
}

inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

template <int ND>
dim3 eik_grid(const GridDesc &g) {
    constexpr int TL = Eik<ND>::TL;
    auto nb = [](int n) { return (unsigned)((n + TL - 1) / TL); };
    return ND == 2 ? dim3(nb(g.nx), nb(g.nz), 1) : dim3(nb(g.nx), nb(g.ny), nb(g.nz));
}
