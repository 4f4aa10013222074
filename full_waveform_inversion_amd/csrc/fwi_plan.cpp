// The decision side of a context (fwi_plan.h): host arithmetic only.  The predicates stand here as they stood beside their
// kernels, measurements included; what each used to read from the environment is now an argument (Hooks).
#include "fwi_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace fwi {

GridDesc make_grid(int ndim, int nz, int ny, int nx, int order, int xpitch_extra) {
    GridDesc g;
    g.ndim = ndim;
    g.nz = nz;
    g.ny = (ndim == 3) ? ny : 1;
    g.nx = nx;
    g.r = order / 2;
    const int hy = (ndim == 3) ? HALO : 0;
    // x pitch: TIGHT -- nx rounded to XALIGN (4: one 16-byte lane) plus ONE halo: the HALO zero cells right of a row are the HALO cells left
    // of the next (nothing writes them).  Every kernel clamps its lanes' addresses into [0, nx] + the halo, so no tile needs
    // slack, and the unused bytes between rows are expensive: until round 3 rows were 4 + roundup(nx, 256) + 4 floats, which
    // cost the 3-D sizes that are not multiples of 256 up to a quarter of their HBM-regime rate (512 x 512 x 384 280 -> 354
    // Gpts/s, 448^3 299 -> 351, 640^3 293 -> 333, 320^3 266 -> 325, 272^3 277 -> 339, 384^3 289 -> 323).  Pitch sweep at 512^3,
    // nx + 8 / 16 / 24 / 32 / 64 / 128 / 256 floats: 350 / 340 / 317 / 305 / 292 / 287 / 276 Gpts/s; nx + 4 against nx + 8: 256^3
    // 424 -> 434, 384^3 301 -> 305.  2-D (cache-resident up to ~4096^2): +1..2 % at every size from 1000^2 to 8192^2.
    // `xpitch_extra` (FWI_XPITCH_EXTRA floats, Hooks::xpitch_extra) is the A/B hook.
    g.sy = HALO + round_up(nx, XALIGN) + std::max(0, xpitch_extra / 4 * 4);
    // (rows whose interior starts on a 128-byte line -- pitch nx + 32 with the gap shared as right / left halo -- were
    // measured as well: 256^3 +2 %, 512^3 +1 %, 640^3 -8 %: not adopted)
    // (sharing the y-halo rows between consecutive planes the same way was measured: within noise, 512^3 349 vs 352)
    const int64_t py = (ndim == 3) ? HALO + round_up(g.ny, YALIGN) + HALO : 1;
    g.sz = g.sy * py;
    g.off0 = (int64_t)HALO * g.sz + (int64_t)hy * g.sy + HALO;
    // 2-D: rows are the tiled axis of step2d_tile, so they are rounded like y is in 3-D.
    // 3-D: LOOKAHEAD extra zero planes behind the far z halo, so the stream kernel's prefetches of
    // planes z + r + 1 ... need no clamping (affine addresses: the plane offsets strength-reduce).
    g.ptot = g.sz * (int64_t)(((ndim == 2) ? round_up(nz, YALIGN) : nz + LOOKAHEAD) + 2 * HALO) + HALO + 2 * MAX_TILE_X;  // (+ the last row's right halo, and
                                        // the edge loads of a 256-column tile whose row ends early: values never used)
    g.cx = (int)round_up(nx, 4);
    g.npts = (int64_t)nz * g.ny * g.cx;
    return g;
}

bool stream_supported(const GridDesc &g, bool is_f32) {
    if (g.nz < 1) return false;
    // any nx: the padded fields and the compact arrays (row stride cx = nx rounded up to 4) keep every
    // lane's 16-byte vector aligned; lanes straddling x = nx compute zeros there (C = 0 in the pad)
    if (is_f32) return true;                  // float4 lanes (3-D stream kernel, 2-D tile kernel)
    return g.ndim == 3;                       // double2 lanes: 3-D stream kernel only
}

bool stream_xpml_supported(const GridDesc &g, const StreamTuning &t, int npml, bool is_f32) {
    if (g.ndim != 3 || !is_f32 || g.r != 4 || npml < 4) return false;
    // (a lane's four cells lie wholly inside or outside the border when npml % 4 == 0; an even npml leaves one lane per
    // side astride the inner edge, whose stores are masked (stream_xpml_partial); the high side's lanes stay 16-byte
    // aligned in the slab row because nx - 2 npml is a multiple of 4)
    if (npml % 2 || g.nx % 4) return false;
    if (g.nx < 2 * (npml + g.r)) return false;         // the two borders (and their reach) do not meet
    const int tw = t.tile_x, nxt = stream_nxt(g, tw);
    // each border and the r cells it reaches into lie inside ONE tile row, i.e. inside one wave
    return tw >= npml + g.r && g.nx - (nxt - 1) * tw >= npml + g.r;
}

StreamTuning stream_default_tuning(const GridDesc &g, bool is_f32, double extra_bytes, bool legacy) {
    const int full_x = is_f32 ? 256 : 128, vl = is_f32 ? 4 : 2;
    // 3-D: split nx into equal x tiles (multiples of the lane vector) rather than full ones plus a remainder
    const int nxt0 = (g.nx + full_x - 1) / full_x;
    const int tile_x = (g.ndim == 2) ? full_x : (int)round_up((g.nx + nxt0 - 1) / nxt0, vl);
    // 2-D: rows per workgroup.  16 is 7 % faster for a lone shot (6.98 vs 7.46 us/step at 1024^2) but
    // 8 co-schedules better when several shots share the GPU (4 concurrent: 3.5 vs 4.4 us/step/shot).
    if (g.ndim == 2) return StreamTuning{8, 1, 1, tile_x};
    // Measured on MI355X (tools/tune_stream.py, tools/size_sweep.py; profiles/r02_stream_tuning_sweep.txt).  Two
    // things decide: every z chunk re-reads 2r halo planes and pays a prologue (~10 planes' worth), so chunks should
    // be long; and workgroups run in rounds of one per CU (256), so the last round should not be a sliver -- a grid
    // whose tiles make 288 columns (768^3 with 8-row tiles) spends its second round on 32 workgroups (235 Gpts/s;
    // 305 with 96-plane chunks = 9 full rounds).  Cost of a candidate (rows per tile, chunks), relative to ideal,
    // with W = the workgroups that saturate the memory system:
    //   (1 + 10 / zchunk) x sum over rounds of max(1, workgroups in the round / W), over (workgroups / W)
    // Two regimes: while the three fields fit the Infinity Cache every CU counts (W = 256) and 4-row tiles cost
    // nothing extra -- their third read of a y row hits in L2; from HBM ~200 workgroups already saturate (W = 200;
    // 384^3 is fastest with 192 workgroups of 192 planes, not with 768 of 48) and the 4-row tile's extra row reads
    // show (200 x 400 x 400: TY 8 x 100 planes 283 Gpts/s, TY 4 x 200 planes 240).  The model reproduces the
    // hand-tuned choices of round 1 (256^3: TY 4 x 64 planes, 407 Gpts/s vs TY 8 x 32 347; 512^3: TY 8 x 256, 328 vs
    // TY 4 x 256 302) and the measured ranking of the chunk lengths at 300^3, 384^3 and 768^3; against the round-1
    // rule (one round, then stop; FWI_STREAM_TUNING=legacy) it changes 700^3 (+39 %) and 768^3 (+24 %) and nothing
    // else from 96^3 to 1024^3.  What it cannot fix: a grid whose columns make 192 - 240 workgroups runs at about
    // that share of the 512^3 rate (384^3: 280 vs 352 Gpts/s) -- per-CU throughput is bounded (neither a deeper
    // prefetch, PF = 2, nor fuller waves, 32-lane rows for 100 % lane use at 384^3, moved it: both measured, both
    // dropped), and shorter chunks to fill more rounds cost more in halo planes than the idle CUs do.
    if (legacy) {
        StreamTuning best{4, g.nz, 1, tile_x};
        for (int ty : {8, 4}) {
            const int64_t tiles_xy = stream_nxt(g, tile_x) * (round_up(g.ny, ty) / ty);
            const int nzc = (int)std::max<int64_t>(1, std::min<int64_t>(g.nz, 256 / std::max<int64_t>(1, tiles_xy)));
            const int zc = std::max((g.nz + nzc - 1) / nzc, std::min(g.nz, 16));
            best = StreamTuning{ty, zc, 1, tile_x};
            if (zc >= 64 || zc >= g.nz) break;  // long enough chunks with 8-row tiles: keep them
        }
        return best;
    }
    constexpr double CUS = 256.0, PROLOGUE = 10.0;
    // (200 MiB: 256^3 = 192 MiB is resident, 272^3 = 230 MiB measurably is not -- it runs 12 % faster tuned as HBM)
    // Round 4: everything the step touches counts, not the three fields alone -- 256^3 with a 16-cell CPML (fields + 50 MB of
    // memory variables + 21 MB of handed-over terms) or in increment form (a fourth field) is an HBM-regime problem and
    // wants the HBM-regime shape: 8-row tiles x 32 planes instead of 4 x 64 (CPML forward 83.3 -> 71.1, adjoint 102.7 -> 93.6
    // us/step on one box; increment form 67.8 / 81.3 / 77.3 -> 63.7 / 76.7 / 75.4) -- once the 8-row x-border variants
    // stopped spilling, that is: in round 3 the same choice measured 116 against 100.
    const bool cache_resident = 3.0 * (double)g.npts * (is_f32 ? 4 : 8) + extra_bytes <= 200.0 * 1024 * 1024;
    // (the kernels that carry extras -- the x border's recursion, the handed-over terms, the increment field -- have a
    // longer dependency chain per plane: every CU counts for them even from HBM.  Measured at 256^3 with the CPML: 8 rows
    // x 32 planes = 256 workgroups 71.6 / 79.8 / 93.7 us/step forward / store / adjoint, x 37 planes = 224 workgroups -- what
    // W = 200 picks -- 81.6 / 97.1 / 100.4, round 3's 4 rows x 64 planes 84.1 / 95.6 / 103.3; at 320^3 one round of 240
    // workgroups 188 against 248 for 320 or 160 of them)
    const double WSAT = (cache_resident || extra_bytes > 0.0) ? 256.0 : 200.0, TY4_PENALTY = cache_resident ? 1.0 : 1.15;
    StreamTuning best{8, g.nz, 1, tile_x};
    double best_cost = 1e30;
    const int zc_min = std::min(g.nz, 16);
    for (int ty : {8, 4}) {
        const int64_t tiles_xy = stream_nxt(g, tile_x) * (round_up(g.ny, ty) / ty);
        int last_zc = 0;
        for (int nzc = 1; nzc <= g.nz; ++nzc) {
            const int zc = (g.nz + nzc - 1) / nzc;
            if (zc < zc_min) break;
            if (zc == last_zc) continue;
            last_zc = zc;
            const double nblk = (double)tiles_xy * ((g.nz + zc - 1) / zc);
            const double full = std::floor(nblk / CUS), rem = nblk - full * CUS;
            const double rounds = full * (CUS / WSAT) + (rem > 0 ? std::max(1.0, rem / WSAT) : 0.0);
            const double cost = (1.0 + PROLOGUE / zc) * rounds / (nblk / WSAT) * (ty == 4 ? TY4_PENALTY : 1.0);
            if (cost < best_cost - 1e-9) {
                best_cost = cost;
                best = StreamTuning{ty, zc, 1, tile_x};
            }
        }
    }
    return best;
}

// Axes (bit mask: z = 1, y = 2) the line form takes for this grid: both or none (the step kernels take the handed-over
// term of both axes together); the slab phases keep the rest.
int pml_line_axes(const GridDesc &g, int npml, bool lines_off) {
    const bool off = lines_off;  // (FWI_NO_PML_LINES, read per context: the tests switch it)
    if (off || g.ndim != 3 || npml < 1) return 0;
    const int nd[2] = {g.nz, g.ny};
    for (int d = 0; d < 2; ++d) {
        constexpr int B = 4;
        const int n = nd[d], r = g.r, W = (2 * r + B - 1) / B * B;
        const int len = n < 2 * npml + 3 * r ? n : npml + r;            // cells of a segment
        const int rows = (len + W + B - 1) / B * B + 3 * r + B;         // table rows the kernel fills
        if (rows > PML_LINE_MAXC || n < 1) return 0;
    }
    return 3;
}

int fused2d_pick_tile(const GridDesc &g, int tile_override) {
    {  // (FWI_FUSED2D_TILE)
        const int v = tile_override;
        if (v == 64 || v == 32 || v == 16) return v;
    }
    // cost of a launch ~ rounds of 256 workgroups x extended tile area (the halo is 4 r = 16 cells whatever the tile:
    // a 32-point tile computes 4x its own area, a 16-point tile 9x -- worth it only while CUs would idle otherwise)
    const int HL = (FUSED2D_STEPS * g.r + 3) / 4 * 4;
    int best = FUSED2D_TILE;
    int64_t best_cost = -1;
    for (int ft : {64, 32, 16}) {
        const int64_t tiles = fused2d_num_tiles(g, ft), e = ft + 2 * HL;
        const int64_t cost = ((tiles + 255) / 256) * e * e;
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            best = ft;
        }
    }
    return best;
}

namespace {

constexpr int cpml_halo(int r) { return (FUSED2D_STEPS * r + 3) / 4 * 4; }

}  // namespace

bool fused2d_cpml_supported(const GridDesc &g, int npml) {
    if (g.ndim != 2 || g.r != 4 || npml < 1) return false;  // (O(8) is what is instantiated)
    const int HL = cpml_halo(g.r), FT = FUSED2D_TILE;
    if (npml > FT - HL) return false;  // the memory-variable images hold 48 border cells
    // Every tile (whole tiles, one overlap seam per axis: fused2d_origin) must see each border either not at all or
    // from a side where nothing but the outside of the grid lies beyond it, and never both borders of an axis
    for (int n : {g.nz, g.nx}) {
        if (n <= FT) return false;
        const int nt = (n + FT - 1) / FT;
        for (int t = 0; t < nt; ++t) {
            const int lo = fused2d_origin(t, n, FT, 1) - HL, hi = lo + FT + 2 * HL;
            const bool low = lo < npml, high = hi > n - npml;  // border cells in the extended region
            if (low && high) return false;
            if (low && lo > 0) return false;     // the low border would begin inside this tile's halo
            if (high && hi < n) return false;    // ... the high border end in it
        }
    }
    return true;
}

void pair3d_default_tuning(const GridDesc &g, int *zchunk, int *tw) {
    // x: one tile for rows of <= 256 columns, else equal tiles of <= 240 interior columns (multiples of 4)
    int t = 256;
    if (g.nx > 256) {
        const int n = (g.nx + 239) / 240;
        t = ((g.nx + n - 1) / n + 3) & ~3;
    }
    *tw = t;
    const int nxt = g.nx <= 256 ? 1 : (g.nx + t - 1) / t;
    const int64_t cols = (int64_t)nxt * ((g.ny + PAIR3D_TY - 1) / PAIR3D_TY);
    // one resident round of workgroups (256 CUs): as few z chunks as that allows (each re-computes 2r planes)
    const int nzc = (int)std::max<int64_t>(1, std::min<int64_t>(g.nz, 256 / std::max<int64_t>(1, cols)));
    *zchunk = std::max((g.nz + nzc - 1) / nzc, std::min(g.nz, 16));
}

bool parse_fixed_placement(const char *s, int k[8]) {
    int n = 0;
    for (;;) {
        char *end = nullptr;
        if (*s < '0' || *s > '9') return false;  // (no sign, no blank: strtol would take them)
        const long v = strtol(s, &end, 10);
        if (v > 7 || n == 8) return false;
        k[n++] = (int)v;
        if (*end == '\0') break;
        if (*end != ',') return false;
        s = end + 1;
    }
    for (; n < 8; ++n) k[n] = k[n - 1];
    return true;
}

Hooks Hooks::from_env() {
    auto number = [](const char *name, int unset) {
        const char *e = getenv(name);
        return e ? atoi(e) : unset;
    };
    // (FWI_XPITCH_EXTRA: the layout A/B hook of DESIGN.md's pitch sweep, read ONCE per process -- not on any hot path)
    static const int xpitch_extra = number("FWI_XPITCH_EXTRA", 0);
    static const bool legacy = getenv("FWI_STREAM_TUNING") && !strcmp(getenv("FWI_STREAM_TUNING"), "legacy");
    Hooks h;
    h.xpitch_extra = xpitch_extra;
    h.stream_legacy = legacy;
    h.stream_pf = number("FWI_STREAM_PF", 0);
    h.stream_ty = number("FWI_STREAM_TY", 0);
    if (getenv("FWI_FUSED2D_SKIPD")) h.fused_skipd = number("FWI_FUSED2D_SKIPD", 0) != 0;
    h.no_fused2d = getenv("FWI_NO_FUSED2D") != nullptr;
    h.no_fused2d_cpml = getenv("FWI_NO_FUSED2D_CPML") != nullptr;
    h.fused_tile = number("FWI_FUSED2D_TILE", 0);
    h.stream_pair = number("FWI_STREAM_PAIR", 0) != 0;
    h.pair_zchunk = number("FWI_PAIR_ZCHUNK", 0);
    h.no_stream_xpml = getenv("FWI_NO_STREAM_XPML") != nullptr;
    h.no_pml_lines = getenv("FWI_NO_PML_LINES") != nullptr;
    if (const char *pt = getenv("FWI_PLACEMENT_TUNE")) h.placement = pt;
    h.debug_pml = getenv("FWI_DEBUG_PML") != nullptr;
    return h;
}

int plan_context(const fwi_config &cfg, const Hooks &hooks, Plan *plan, std::string *why) {
    Plan p;
    const bool f32 = cfg.dtype == FWI_F32;
    p.gd = make_grid(cfg.ndim, cfg.nz, cfg.ny, cfg.nx, cfg.order, hooks.xpitch_extra);
    const bool can_stream = stream_supported(p.gd, f32);
    if (cfg.kernel == FWI_KERNEL_STREAM && !can_stream) {
        *why = "STREAM kernel: fp64 is 3-D only";
        return FWI_EINVAL;
    }
    // the increment form exists in the 3-D fp32 stream kernel and in the point kernel
    const bool inc_point = cfg.update_form == FWI_UPDATE_INCREMENT && !(cfg.ndim == 3 && f32);
    if (inc_point && cfg.kernel == FWI_KERNEL_STREAM) {
        *why = "update_form increment: the STREAM kernel takes it for 3-D fp32 only";
        return FWI_EINVAL;
    }
    p.esize = f32 ? 4 : 8;
    p.ckpt = cfg.ckpt_interval;
    p.istride = cfg.image_stride > 1 ? cfg.image_stride : 1;
    p.inc = cfg.update_form == FWI_UPDATE_INCREMENT;
    p.cpml = cfg.abc == FWI_ABC_CPML && cfg.npml > 0;
    p.qbf16 = cfg.store_dtype == FWI_STORE_BF16;
    p.qes = p.qbf16 ? 2 : p.esize;
    p.kernel = (cfg.kernel == FWI_KERNEL_POINT || !can_stream || inc_point) ? K_POINT : K_STREAM;
    if (p.kernel == K_STREAM) {
        // what a time step touches beside the three fields: the increment field; the CPML's memory variables (psi, zeta
        // over 2 npml planes per axis) and the handed-over border terms (two shells of npml + r)
        double extra = p.inc ? (double)p.gd.ptot * p.esize : 0.0;
        if (p.cpml && cfg.ndim == 3) {
            const double face[3] = {(double)p.gd.ny * p.gd.cx, (double)p.gd.nz * p.gd.cx, (double)p.gd.nz * p.gd.ny};
            for (int d = 0; d < 3; ++d) extra += 2.0 * std::min(2 * cfg.npml, d == 0 ? cfg.nz : d == 1 ? cfg.ny : cfg.nx) * face[d] * p.esize;
            for (int d = 0; d < 2; ++d) extra += 2.0 * (cfg.npml + p.gd.r) * face[d] * p.esize;
        }
        p.tune = stream_default_tuning(p.gd, f32, extra, hooks.stream_legacy);
        if (cfg.zchunk > 0) p.tune.zchunk = cfg.zchunk;
        if (hooks.stream_pf >= 1 && hooks.stream_pf <= 3) p.tune.pf = hooks.stream_pf;  // tuning hook: prefetch depth in planes
        const int ty = hooks.stream_ty;                                                  // tuning hook: rows per workgroup
        if (ty == 4 || ty == 8 || (ty == 16 && cfg.ndim == 2)) p.tune.ty = ty;
    }
    // 2-D fp32 grids: advance FUSED2D_STEPS time steps per launch (fwi_fused2d.hip) whenever the step
    // count allows it (FWI_NO_FUSED2D is the tuning / comparison hook)
    // (CPML: the fused kernel carries the border recursion itself where the tiling admits it, fused2d_cpml_supported;
    // otherwise the slab kernels run between time steps: one step per launch, the tile kernel.  FWI_NO_FUSED2D_CPML is
    // the comparison hook)
    // Increment form in 2-D: the fused kernel carries it (same traffic as the standard form); the steps it cannot take
    // (step counts off the multiple of 4) go through the point kernel, which Plan::kernel names in that case.
    p.fused_skipd = hooks.fused_skipd;  // tuning / test hook
    const bool cpml_in_launch = p.cpml && !p.inc && p.kernel == K_STREAM && fused2d_cpml_supported(p.gd, cfg.npml) &&
                                !hooks.no_fused2d_cpml;
    p.fused2d = cfg.ndim == 2 && f32 && (!p.cpml || cpml_in_launch) && !hooks.no_fused2d &&
                (p.inc ? cfg.kernel == FWI_KERNEL_AUTO : p.kernel == K_STREAM);
    if (p.fused2d && !p.cpml && !p.inc) p.fused_ft = fused2d_pick_tile(p.gd, hooks.fused_tile);
    // 3-D fp32 stream contexts: two time steps per pass for forward sweeps without imaging (FWI_STREAM_PAIR=0 /
    // =1 is the tuning / comparison hook)
    if (cfg.ndim == 3 && f32 && p.kernel == K_STREAM && !p.inc && !p.cpml) {
        p.pair3d = hooks.stream_pair && cfg.npml == 0;  // (the two-step kernel exists undamped only)
        if (p.pair3d) {
            pair3d_default_tuning(p.gd, &p.pair_zc, &p.pair_tw);
            if (hooks.pair_zchunk >= 1) p.pair_zc = hooks.pair_zchunk;
        }
    }
    // CPML in 3-D: the z / y borders run as ONE line launch before every step, which hands their term to the step kernel
    // (both axes or none); with it the 3-D fp32 O(8) stream kernel carries the x border's recursion in its own lanes.
    // Whatever is left runs as slab phases around the step kernel.
    if (p.cpml && cfg.ndim == 3) p.pml_lines = pml_line_axes(p.gd, cfg.npml, hooks.no_pml_lines);
    p.xpml = p.cpml && p.kernel == K_STREAM && p.pml_lines == 3 && !hooks.no_stream_xpml &&
             stream_xpml_supported(p.gd, p.tune, cfg.npml, f32);
    // 3-D CPML contexts past the cache-resident sizes place their small arrays by measurement (Impl::tune_placement).
    // FWI_PLACEMENT_TUNE: "0" = off, "pad" = padded allocations without the search (A/B hooks), "force" = also on grids
    // below the size threshold (tests: the oracle comparisons run small grids), "fixed:<k0>,<k1>,..." = on any grid, NO
    // search: movable array i (in the search order) sits k_i * 2 MiB into its allocation, the last value repeats (tests:
    // a layout that is asked for instead of timed; 0 <= k <= 7, anything else is FWI_EINVAL).  A context that places
    // nothing ignores "fixed:" as it ignores "force".
    const std::string &pt = hooks.placement;
    const bool place_fixed = !pt.compare(0, 6, "fixed:");
    const bool place_on = f32 && cfg.ndim == 3 && p.kernel == K_STREAM && pt != "0" &&
                          ((double)p.gd.ptot * p.esize >= 48e6 || pt == "force" || place_fixed);
    if (place_on && p.xpml) p.place_kind = 1;
    else if (place_on && p.inc && !p.cpml) p.place_kind = 2;
    if (p.place_kind) {
        p.place_pad = (size_t)14 << 20;
        p.place_mode = place_fixed ? PLACE_FIXED : pt == "pad" ? PLACE_PAD : PLACE_SEARCH;
    }
    *plan = p;
    // (the syntax of "fixed:" matters only to a context that places)
    if (p.place_mode == PLACE_FIXED && !parse_fixed_placement(pt.c_str() + 6, plan->fixed_k)) {
        *why = "FWI_PLACEMENT_TUNE=fixed:<k0>,<k1>,...: one to eight offsets, each 0 ... 7 (units of 2 MiB)";
        return FWI_EINVAL;
    }
    return FWI_OK;
}

void plan_report(const Plan &p, char *buf, size_t len) {
    snprintf(buf, len, "fwi: cpml=%d fused2d=%d pair3d=%d x-in-kernel=%d line-axes=%d (ty %d zchunk %d)", (int)p.cpml,
             (int)p.fused2d, (int)p.pair3d, (int)p.xpml, p.pml_lines, p.tune.ty, p.tune.zchunk);
}

const char *plan_kernel_name(const Plan &p) {
    if (p.fused2d) return "step2d_fused";
    if (p.kernel == K_STREAM && p.gd.ndim == 2) return "step2d_tile";
    if (p.kernel == K_STREAM) return "step3d_stream";
    return "step_point";
}

}  // namespace fwi
