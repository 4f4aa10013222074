// What the host units of the eikonal calls share (fwi_api_eikonal.hip, fwi_api_eikonal_stage.hip): the checks of a node
// list, the number of inner sweeps, the upload of a point list and the launch loop of the block-Jacobi iterations with
// its stopping rule.  Not a header for other code: include it inside the unit's anonymous namespace, after fwi_host.h,
// fwi_eikonal.h and <algorithm>, <cmath>, <cstdlib>, <vector>.
#pragma once

constexpr int EIK_BATCH = 4;  // launches between two reads of the change flags

// node coordinates (n, ndim) in grid order -> compact indices; FWI_EINVAL for a node outside the grid (and, with
// `unique`, for one listed twice)
int compact_nodes(fwi_ctx *ctx, const char *who, const char *what, int64_t n, const int32_t *idx, bool unique,
                  std::vector<int64_t> &out) {
    const GridDesc &g = ctx->gd;
    const int nd = g.ndim;
    out.resize((size_t)n);
    for (int64_t k = 0; k < n; ++k) {
        const int32_t *p = idx + k * nd;
        const int z = p[0], y = nd == 3 ? p[1] : 0, x = p[nd - 1];
        if (z < 0 || z >= g.nz || y < 0 || y >= g.ny || x < 0 || x >= g.nx)
            return ctx->fail(FWI_EINVAL, "%s: %s[%lld] lies outside the grid", who, what, (long long)k);
        out[(size_t)k] = ((int64_t)z * g.ny + y) * g.cx + x;
    }
    if (unique && n > 1) {
        std::vector<int64_t> s(out);
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end())
            return ctx->fail(FWI_EINVAL, "%s: %s names a node twice", who, what);
    }
    return FWI_OK;
}

int inner_sweeps(const fwi_ctx *ctx) {
    // FWI_EIKONAL_K: inner sweeps per launch (tuning / tests), read at every call
    const char *e = getenv("FWI_EIKONAL_K");
    const int k = e ? atoi(e) : 0;
    return (k >= 1 && k <= EIK_KMAX) ? k : eik_default_k(ctx->gd);
}

template <typename T>
struct EikHost {
    // idx -> ctx->eik_idx, values (as T) -> ctx->eik_val
    static int upload_points(fwi_ctx *ctx, const std::vector<int64_t> &idx, const double *val) {
        const size_t n = idx.size();
        int rc = ensure(ctx, ctx->eik_idx, n * sizeof(int64_t));
        if (rc || (rc = upload_series(ctx, ctx->eik_idx.p, idx.data(), n * sizeof(int64_t)))) return rc;
        if (!val) return FWI_OK;
        std::vector<T> v(n);
        for (size_t k = 0; k < n; ++k) v[k] = (T)val[k];
        if ((rc = ensure(ctx, ctx->eik_val, n * sizeof(T))) || (rc = upload_series(ctx, ctx->eik_val.p, v.data(), n * sizeof(T))))
            return rc;
        return FWI_OK;  // (upload_series has copied v into the context's staging buffer)
    }

    // Launches `step(in, out, flag)` from `a` into `b` and back until one changes nothing (then a == b on the grid) or
    // the cap is reached (FWI_ESTATE; the newest iterate is left in a).  The flags are read every EIK_BATCH launches;
    // the count reported is that of the first launch that changed nothing, whatever the batch.
    template <typename Step>
    static int iterate(fwi_ctx *ctx, const char *who, T *a, T *b, int32_t max_sweeps, int32_t *launches_out, Step step) {
        const GridDesc &g = ctx->gd;
        const int K = inner_sweeps(ctx);
        const int64_t cap = max_sweeps > 0 ? max_sweeps : 4 * ((int64_t)g.nz + (g.ndim == 3 ? g.ny : 0) + g.nx);
        const int64_t max_launches = (cap + K - 1) / K;
        int rc = ensure(ctx, ctx->eik_flags, EIK_BATCH * sizeof(int));
        if (rc) return rc;
        int *flags = (int *)ctx->eik_flags.p;
        T *in = a, *out = b;
        int64_t done = 0;
        while (done < max_launches) {
            const int nb = (int)std::min<int64_t>(EIK_BATCH, max_launches - done);
            int host[EIK_BATCH];
            HIPCHK(ctx, hipMemsetAsync(flags, 0, nb * sizeof(int), ctx->stream));
            for (int i = 0; i < nb; ++i) {
                HIPCHK(ctx, step(in, out, K, flags + i));
                std::swap(in, out);
            }
            HIPCHK(ctx, hipMemcpyAsync(host, flags, nb * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            for (int i = 0; i < nb; ++i)
                if (!host[i]) {
                    if (launches_out) *launches_out = (int32_t)(done + i + 1);
                    return FWI_OK;
                }
            done += nb;
        }
        if (in != a) HIPCHK(ctx, hipMemcpyAsync(a, in, (size_t)g.npts * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (launches_out) *launches_out = (int32_t)done;
        return ctx->fail(FWI_ESTATE, "%s: still changing after %lld launches of %d sweeps (max_sweeps = %lld)", who,
                         (long long)done, K, (long long)cap);
    }
};

// the init list of fwi_eikonal / fwi_eikonal_gradient: FWI_EINVAL unless it is non-empty, inside the grid, listed once
// per node and its distances are finite and >= 0
int init_list(fwi_ctx *ctx, const char *who, int32_t n, const int32_t *idx, const double *dist, const int32_t *ref,
              std::vector<int64_t> &nodes, int64_t *ref_out) {
    if (n < 1) return ctx->fail(FWI_EINVAL, "%s: the init list is empty (n_init = %d)", who, (int)n);
    if (!idx || !dist || !ref) return ctx->fail(FWI_EINVAL, "%s: null %s", who, !idx ? "init_idx" : !dist ? "init_dist" : "ref_idx");
    for (int32_t k = 0; k < n; ++k)
        if (!std::isfinite(dist[k]) || dist[k] < 0.0)
            return ctx->fail(FWI_EINVAL, "%s: init_dist[%d] = %g must be finite and >= 0", who, (int)k, dist[k]);
    std::vector<int64_t> r;
    int rc = compact_nodes(ctx, who, "ref_idx", 1, ref, false, r);
    if (rc || (rc = compact_nodes(ctx, who, "init_idx", n, idx, true, nodes))) return rc;
    *ref_out = r[0];
    return FWI_OK;
}
