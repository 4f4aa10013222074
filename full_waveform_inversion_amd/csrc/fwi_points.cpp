// A shot's point tables (fwi_points.h): integer geometry only.
#include "fwi_points.h"

#include <algorithm>

namespace fwi {

namespace {

struct Zyx {
    int z, y, x;
};
inline Zyx point(const GridDesc &g, const int32_t *idx, int i) {
    const int32_t *t = idx + (size_t)i * g.ndim;
    return {t[0], g.ndim == 3 ? t[1] : 0, t[g.ndim - 1]};
}

// run[k] = length of the run of equal entries that starts at k, 0 where k continues one; same(a, b): a and b are of one run
template <typename Same>
std::vector<int> run_lengths(int n, Same same) {
    std::vector<int> run(n, 0);
    for (int k = n - 1, len = 0; k >= 0; --k) {
        len = (k + 1 < n && same(k, k + 1)) ? len + 1 : 1;
        run[k] = (k == 0 || !same(k - 1, k)) ? len : 0;
    }
    return run;
}

}  // namespace

int flatten(const GridDesc &g, const int32_t *idx, int n, FlatPoints *out) {
    out->pidx.resize(n);
    out->cidx.resize(n);
    for (int i = 0; i < n; ++i) {
        const Zyx p = point(g, idx, i);
        if (p.z < 0 || p.z >= g.nz || p.y < 0 || p.y >= g.ny || p.x < 0 || p.x >= g.nx) return i;
        out->pidx[i] = g.off0 + (int64_t)p.z * g.sz + (int64_t)p.y * g.sy + p.x;
        out->cidx[i] = ((int64_t)p.z * g.ny + p.y) * g.cx + p.x;
    }
    return -1;
}

// (the kernels' block decode: bx = bid % nxt, then rows of ty, then chunks of zchunk planes)
int stream_tile_of(const GridDesc &g, const StreamTuning &t, int z, int y, int x) {
    const int nxt = stream_nxt(g, t.tile_x);
    if (g.ndim == 2) return (z / t.ty) * nxt + x / t.tile_x;
    const int nyt = (g.ny + t.ty - 1) / t.ty;
    return ((z / t.zchunk) * nyt + y / t.ty) * nxt + x / t.tile_x;
}

int stream_num_tiles(const GridDesc &g, const StreamTuning &t) {
    const int nxt = stream_nxt(g, t.tile_x);
    if (g.ndim == 2) return nxt * ((g.nz + t.ty - 1) / t.ty);
    return nxt * ((g.ny + t.ty - 1) / t.ty) * ((g.nz + t.zchunk - 1) / t.zchunk);
}

// (step_point: 64 columns x 4 rows; the rows are y in 3-D, one plane per workgroup, and z in 2-D)
int point_tile_of(const GridDesc &g, int z, int y, int x) {
    const int nbx = (g.nx + 63) / 64;
    return g.ndim == 3 ? (z * ((g.ny + 3) / 4) + y / 4) * nbx + x / 64 : (z / 4) * nbx + x / 64;
}

int point_num_tiles(const GridDesc &g) {
    const int nbx = (g.nx + 63) / 64;
    return g.ndim == 3 ? nbx * ((g.ny + 3) / 4) * g.nz : nbx * ((g.nz + 3) / 4);
}

void step_table(const Plan &plan, const int32_t *idx, int n, const FlatPoints &flat, StepTable *out) {
    const GridDesc &g = plan.gd;
    const bool st = plan.kernel == K_STREAM;
    const int ntile = st ? stream_num_tiles(g, plan.tune) : point_num_tiles(g);
    out->start.assign(ntile + 1, 0);
    std::vector<int> tile(n);
    for (int i = 0; i < n; ++i) {
        const Zyx p = point(g, idx, i);
        tile[i] = st ? stream_tile_of(g, plan.tune, p.z, p.y, p.x) : point_tile_of(g, p.z, p.y, p.x);
        ++out->start[tile[i] + 1];
    }
    for (int k = 0; k < ntile; ++k) out->start[k + 1] += out->start[k];
    std::vector<int> &col = out->col;
    col.resize(n);
    for (int i = 0; i < n; ++i) col[i] = i;
    std::stable_sort(col.begin(), col.end(), [&](int a, int b) {
        return tile[a] != tile[b] ? tile[a] < tile[b] : flat.pidx[a] < flat.pidx[b];
    });
    out->pidx.resize(n);
    out->cidx.resize(n);
    for (int k = 0; k < n; ++k) {
        out->pidx[k] = flat.pidx[col[k]];
        out->cidx[k] = flat.cidx[col[k]];
    }
    out->run = run_lengths(n, [&](int a, int b) { return out->pidx[a] == out->pidx[b] && tile[col[a]] == tile[col[b]]; });
}

void fused2d_tables(const Plan &plan, const int32_t *idx, int n, Fused2dTables *out) {
    const GridDesc &g = plan.gd;
    const int FT = plan.fused_ft;
    const int HL = (FUSED2D_STEPS * g.r + 3) / 4 * 4;  // as in step2d_fused
    const int ntx = (g.nx + FT - 1) / FT, ntz = (g.nz + FT - 1) / FT, ntile = ntx * ntz;
    const int seam = plan.cpml ? 1 : 0;
    struct Ent {
        int tile, lz, lx, col;
        unsigned char interior;
    };
    struct Ax {
        int t, l;
        bool own;
    };
    auto tiles_of = [&](int c, int nn, int nt, Ax *ax) {  // tiles whose extended region holds coordinate c
        int m = 0;
        // HL <= FT and the seam shifts a tile by less than FT: the owning tile's index is within 2 of c / FT
        for (int t = std::max(0, c / FT - 1); t <= std::min(nt - 1, c / FT + 2); ++t) {
            const int o = fused2d_origin(t, nn, FT, seam);
            if (c < o - HL || c >= o + FT + HL) continue;
            const int lo = fused2d_own(t, nn, FT, seam), hi = t + 1 < nt ? fused2d_own(t + 1, nn, FT, seam) : nn;
            ax[m++] = Ax{t, c - (o - HL), c >= lo && c < hi};
        }
        return m;
    };
    std::vector<Ent> ents;
    for (int i = 0; i < n; ++i) {
        const Zyx p = point(g, idx, i);
        Ax az[4], ax[4];
        const int mz = tiles_of(p.z, g.nz, ntz, az), mx = tiles_of(p.x, g.nx, ntx, ax);
        for (int a = 0; a < mz; ++a)
            for (int b = 0; b < mx; ++b)
                ents.push_back({az[a].t * ntx + ax[b].t, az[a].l, ax[b].l, i, (unsigned char)(az[a].own && ax[b].own)});
    }
    std::stable_sort(ents.begin(), ents.end(), [](const Ent &a, const Ent &b) {
        if (a.tile != b.tile) return a.tile < b.tile;
        return a.lz != b.lz ? a.lz < b.lz : a.lx < b.lx;  // a node's entries consecutive, in entry order
    });
    out->start.assign(ntile + 1, 0);
    out->rstart.assign(ntile + 1, 0);
    for (const Ent &e : ents) {
        ++out->start[e.tile + 1];
        out->lz.push_back(e.lz);
        out->lx.push_back(e.lx);
        out->col.push_back(e.col);
        out->interior.push_back(e.interior);
        if (!e.interior) continue;
        ++out->rstart[e.tile + 1];
        out->rlz.push_back(e.lz);
        out->rlx.push_back(e.lx);
        out->rcol.push_back(e.col);
    }
    for (int k = 0; k < ntile; ++k) {
        out->start[k + 1] += out->start[k];
        out->rstart[k + 1] += out->rstart[k];
    }
    out->run = run_lengths((int)ents.size(), [&](int a, int b) {
        return ents[a].tile == ents[b].tile && ents[a].lz == ents[b].lz && ents[a].lx == ents[b].lx;
    });
}

void pair3d_table(const Plan &plan, const int32_t *idx, int n, Pair3dTable *out) {
    const GridDesc &g = plan.gd;
    const int zc = plan.pair_zc, tw = plan.pair_tw, r = g.r, TYI = PAIR3D_TY;
    const int nxt = g.nx <= 256 ? 1 : (g.nx + tw - 1) / tw;  // as launch_pair3d
    const int nyt = (g.ny + TYI - 1) / TYI, nzc = (g.nz + zc - 1) / zc;
    const int ntile = nxt * nyt * nzc;
    std::vector<std::vector<Pair3dInj>> per(ntile);
    for (int i = 0; i < n; ++i) {
        const Zyx p = point(g, idx, i);
        for (int bz = std::max(0, (p.z - r) / zc - 1); bz < nzc; ++bz) {
            const int z0 = bz * zc, z1 = std::min(g.nz, z0 + zc);
            if (p.z < z0 - r || p.z >= z1 + r) continue;
            for (int by = std::max(0, (p.y - r) / TYI - 1); by < nyt; ++by) {
                const int y0 = by * TYI;
                if (p.y < y0 - r || p.y >= y0 + TYI + r) continue;
                for (int bx = 0; bx < nxt; ++bx) {
                    const int xi0 = bx * tw, xbase = nxt == 1 ? 0 : xi0 - 2 * HALO;  // lane 0's first column
                    if (nxt > 1 && (p.x < xi0 - r || p.x >= xi0 + tw + r)) continue;
                    const bool own = p.z >= z0 && p.z < z1 && p.y >= y0 && p.y < y0 + TYI &&
                                     (nxt == 1 || (p.x >= xi0 && p.x < xi0 + tw));
                    per[(bz * nyt + by) * nxt + bx].push_back(Pair3dInj{p.z, p.y - y0, p.x - xbase, i, 0.f, own ? 1 : 0});
                }
            }
        }
    }
    out->start.assign(ntile + 1, 0);
    out->ent.clear();
    for (int k = 0; k < ntile; ++k) {
        out->start[k + 1] = out->start[k] + (int)per[k].size();
        out->ent.insert(out->ent.end(), per[k].begin(), per[k].end());
    }
}

SpreadOwners spread_owners(int npts, int nnodes, const int32_t *pt_start, bool have_weight) {
    SpreadOwners so;
    auto refuse = [&](SpreadCheck c, int point = -1, int count = 0) {
        so.check = c;
        so.point = point;
        so.count = count;
        return so;
    };
    if (npts < 0 || (npts > 0 && (!pt_start || !have_weight))) return refuse(SPREAD_BAD_SET);
    if (npts == 0) return refuse(nnodes != 0 ? SPREAD_NODES_WITHOUT_POINTS : SPREAD_OK);
    if (pt_start[0] != 0 || pt_start[npts] != nnodes) return refuse(SPREAD_BAD_RANGE);
    // (every count is checked before an owner is written: counts of 0 .. 8 that run from 0 to nnodes stay inside it)
    for (int p = 0; p < npts; ++p) {
        const int64_t count = (int64_t)pt_start[p + 1] - pt_start[p];
        if (count < 0 || count > 8) return refuse(SPREAD_BAD_COUNT, p, (int)count);
    }
    so.owner.resize((size_t)nnodes);
    for (int p = 0; p < npts; ++p)
        for (int m = pt_start[p]; m < pt_start[p + 1]; ++m) so.owner[m] = p;
    return so;
}

}  // namespace fwi
