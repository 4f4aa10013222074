// Device functions shared by the eikonal kernels (fwi_eikonal.hip) and the tangent kernels (fwi_eikonal_tangent.hip):
// the tile geometry, THE local solver and the weights derived from it.  Every kernel of either unit takes G, "T_i < G_i"
// and the upwind choice from here, so the two units cannot disagree on a decision of the arithmetic.  At the end, the two host helpers
// that size the launches of both units (blocks256, eik_grid).  Not a header for other code:
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

inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

template <int ND>
dim3 eik_grid(const GridDesc &g) {
    constexpr int TL = Eik<ND>::TL;
    auto nb = [](int n) { return (unsigned)((n + TL - 1) / TL); };
    return ND == 2 ? dim3(nb(g.nx), nb(g.nz), 1) : dim3(nb(g.nx), nb(g.ny), nb(g.nz));
}
