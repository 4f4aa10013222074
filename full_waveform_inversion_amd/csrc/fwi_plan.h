// Which path a context takes, decided from its configuration and the creation-time hooks alone: the padded layout, the
// step kernel and its launch shape, the temporal blocking, where the CPML's borders run and what the placement search may
// move.  Plain C++ (no HIP, no device): fwi_create validates, asks plan_context, then allocates; tests/plan_host.cpp asks
// the same function on the CPU.  The geometry and the constants that the decisions share with the kernels are defined
// here once; fwi_kernels.h includes this header.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/fwi.h"

#ifdef __HIP__
#define FWI_HD __host__ __device__
#else
#define FWI_HD
#endif

namespace fwi {

// Layout halo of every padded field: 4 cells on each side of every stencil
// axis, whatever the order (4 floats = 16 B keeps interior rows float4-aligned).
constexpr int HALO = 4;
// Padded extents: x to XALIGN cells plus one shared halo (tight rows: slack between rows costs HBM efficiency, make_grid),
// y to YALIGN rows.
constexpr int XALIGN = 4;
constexpr int YALIGN = 16;
// Zero planes appended behind the far z halo of 3-D fields: the stream kernel reads up to
// r + PF (<= 4 + 3) planes past the last interior plane without clamping.
constexpr int LOOKAHEAD = 4;

// Padded field geometry.  Element (z, y, x) of the interior lives at
// off0 + z*sz + y*sy + x.  2-D grids are ny = 1 with no y halo (sz == sy).
struct GridDesc {
    int ndim, nz, ny, nx;
    int cx;          // row stride of COMPACT arrays: nx rounded up to 4, so that rows stay 16-byte
                     // aligned for any nx; the cx - nx pad columns hold zeros
    int r;           // stencil radius (order / 2)
    int64_t sy, sz;  // padded strides in elements (x stride is 1)
    int64_t off0;    // padded offset of interior point (0, 0, 0)
    int64_t ptot;    // elements of one padded field
    int64_t npts;    // nz * ny * cx: elements of one compact array (pad columns included)
};

// `xpitch_extra`: floats of slack added to the (tight) x pitch -- the A/B hook behind DESIGN.md's pitch sweep
// (Hooks::xpitch_extra; it is not consulted on any other path).
GridDesc make_grid(int ndim, int nz, int ny, int nx, int order, int xpitch_extra = 0);
// Widest x tile of any step kernel in elements (64 lanes x one float4): the tail behind the last row of a padded field
// covers the edge loads of such a tile whose row ends early (values never used).
constexpr int MAX_TILE_X = 256;

enum StencilKernel { K_POINT = 1, K_STREAM = 2 };

struct StreamTuning {
    int ty;      // rows per workgroup (4 or 8)
    int zchunk;  // planes marched per workgroup
    int pf;      // planes fetched ahead of use (1..3)
    int tile_x;  // x extent of a tile in elements: at most 64 lanes x one 16-byte vector (256 fp32 /
                 // 128 fp64); the 3-D kernel takes narrower, equal tiles when nx is not a multiple of that
};

inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
// x tiles of `tile_x` elements: 64 lanes x one 16-byte vector (256 floats / 128 doubles)
inline int stream_nxt(const GridDesc &g, int tile_x) { return (int)(round_up(g.nx, tile_x) / tile_x); }

// True when the stream kernel supports this grid / dtype.
bool stream_supported(const GridDesc &g, bool is_f32);
// `extra_bytes`: what a time step touches beside the three padded fields (the increment form's fourth field, the CPML's
// memory variables and handed-over terms): it decides whether the step is Infinity-Cache resident, i.e. which regime the
// launch shape is chosen for.  `legacy`: the round-1 rule (Hooks::stream_legacy).
StreamTuning stream_default_tuning(const GridDesc &g, bool is_f32, double extra_bytes = 0.0, bool legacy = false);

// ---- convolutional PML ------------------------------------------------------------------------------------------
// The SHELL of an axis of n cells: its two borders and the r cells inward that their term reaches (the rows whose
// update takes a CPML term of that axis).  When the two shells meet (n < 2 npml + 3 r, the line kernel's one-segment
// case) the shell is the whole axis.  Rows are numbered low border first.
FWI_HD inline int pml_shell_rows(int n, int npml, int r) { return n < 2 * npml + 3 * r ? n : 2 * (npml + r); }
constexpr int PML_LINE_MAXC = 192;  // rows of the line kernel's coefficient tables (pml_line_axes checks)
// pml_line_axes: the axes (z = 1, y = 2) the line form of the z / y border takes for this grid -- the slab phases are then
// run without them.  `lines_off`: none (Hooks::no_pml_lines).
int pml_line_axes(const GridDesc &g, int npml, bool lines_off);
// True when the 3-D stream kernel can carry the x border's recursion in its lanes (see step3d_stream, XP)
bool stream_xpml_supported(const GridDesc &g, const StreamTuning &t, int npml, bool is_f32);

// ---- 2-D temporal blocking (fwi_fused2d.hip): FUSED2D_STEPS time steps per launch ----------------
constexpr int FUSED2D_STEPS = 4;   // time steps advanced per launch
constexpr int FUSED2D_TILE = 64;   // interior tile edge (points) of a grid that fills the chip with such tiles; extended
                                   // edge = TILE + 2 STEPS r.  Smaller grids take 32- or 16-point tiles (Fused2dArgs::ft)

// Tiling of an axis of n cells by WHOLE tiles of ft cells with one overlap seam in the middle -- the fused 2-D kernel
// with the CPML inside, whose border tiles must be whole (the recursion reaches 2 r cells per sub-step, so a border cell
// may not sit in a tile's halo): the lower half of the tiles starts at t * ft, the upper half is anchored at the high
// end (origins rounded up to a 16-byte group; the last tile may overhang n by <= 3 cells like any partial tile), and the
// two tiles either side of the seam overlap by nt * ft - n cells in the interior of the grid, which both compute and
// the lower one stores.  `seam` = 0: the plain tiling t * ft.  fused2d_own: the first cell of tile t that t owns.
FWI_HD inline int fused2d_origin(int t, int n, int ft, int seam) {
    const int nt = (n + ft - 1) / ft;
    return (!seam || nt < 2 || t < nt / 2) ? t * ft : ((n - (nt - t) * ft + 3) & ~3);
}
FWI_HD inline int fused2d_own(int t, int n, int ft, int seam) {
    return t == 0 ? 0 : fused2d_origin(t - 1, n, ft, seam) + ft;  // (= the tile's origin except just above the seam)
}
inline int fused2d_num_tiles(const GridDesc &g, int ft = FUSED2D_TILE) {
    return ((g.nx + ft - 1) / ft) * ((g.nz + ft - 1) / ft);
}
// Tile edge that minimises rounds of workgroups x extended tile area (a 512^2 grid makes 64 tiles of 64^2 -- a
// quarter of the chip -- but 256 of 32^2); `tile_override` = 64, 32 or 16 is taken as it is (Hooks::fused_tile).
int fused2d_pick_tile(const GridDesc &g, int tile_override);
// True when the fused kernel can carry the CPML of this grid: every border cell a tile sees lies deep inside that
// tile's extended region or against the outside of the grid (conditions at fused2d_cpml_supported).
bool fused2d_cpml_supported(const GridDesc &g, int npml);

// ---- 3-D temporal blocking (fwi_pair3d.hip): two time steps per pass, fp32, forward sweeps without imaging ----
constexpr int PAIR3D_TY = 8;   // interior rows (= waves) per workgroup
void pair3d_default_tuning(const GridDesc &g, int *zchunk, int *tw);
struct Pair3dInj {             // one source term as seen by one workgroup (built by pair3d_table, fwi_points.h)
    int z, yoff, xoff;         // plane; row relative to the tile's first interior row; column relative to lane 0's
    int col;                   // column of the amplitude rows
    float cu;                  // coefficient of the amplitude in u
    int interior;              // the point is one of the workgroup's own (then step 2 injects it too)
};

// FWI_PLACEMENT_TUNE=fixed:<k0>,<k1>,... : one to eight offsets in units of 2 MiB, each within the
// 14 MiB of slack (0 ... 7); the last one repeats for the arrays that are not listed
bool parse_fixed_placement(const char *s, int k[8]);

// ---- the plan -------------------------------------------------------------------------------------------------
// Every creation-time hook, as the environment states it.  Values outside a hook's range are kept here and ignored by
// plan_context, silently, as they always were.  The launch-time hooks (FWI_FUSED2D_NO_TILE_ORDER, FWI_FUSED2D_NOREMAP,
// FWI_STREAM_NOREMAP, FWI_PML_LINE_VL, FWI_EIKONAL_K) decide no path and stay with their launchers.
struct Hooks {
    int xpitch_extra = 0;          // FWI_XPITCH_EXTRA: floats of slack in the x pitch (make_grid); once per process
    bool stream_legacy = false;    // FWI_STREAM_TUNING=legacy: the round-1 launch shape; once per process
    int stream_pf = 0;             // FWI_STREAM_PF: prefetch depth in planes, 1 ... 3
    int stream_ty = 0;             // FWI_STREAM_TY: rows per workgroup, 4 or 8 (2-D: or 16)
    int fused_skipd = -1;          // FWI_FUSED2D_SKIPD: Fused2dArgs::skipd forced to 0 / 1 (-1 = by tile count)
    bool no_fused2d = false;       // FWI_NO_FUSED2D: one step per launch in 2-D
    bool no_fused2d_cpml = false;  // FWI_NO_FUSED2D_CPML: the 2-D CPML as slab launches around the tile kernel
    int fused_tile = 0;            // FWI_FUSED2D_TILE: 64, 32 or 16
    bool stream_pair = false;      // FWI_STREAM_PAIR (non-zero): two steps per pass on undamped 3-D fp32 forward sweeps
    int pair_zchunk = 0;           // FWI_PAIR_ZCHUNK: planes per workgroup of that kernel, >= 1
    bool no_stream_xpml = false;   // FWI_NO_STREAM_XPML: the x border as slab phases around the step kernel
    bool no_pml_lines = false;     // FWI_NO_PML_LINES: the z / y borders as slab phases
    std::string placement;         // FWI_PLACEMENT_TUNE: "0", "pad", "force", "fixed:<k0>,..." (include/fwi.h); "" = unset
    bool debug_pml = false;        // FWI_DEBUG_PML: fwi_create writes plan_report's line to stderr
    // The first two are read when the first context of the process is created, the others on every call (the tests
    // switch them between contexts of one process).
    static Hooks from_env();
};

enum PlaceMode { PLACE_OFF = 0, PLACE_PAD, PLACE_SEARCH, PLACE_FIXED };

// What fwi_create decides before it allocates anything (fwi_ctx derives from it)
struct Plan {
    GridDesc gd{};
    int kernel = K_POINT;
    StreamTuning tune{8, 0, 1, 256};
    size_t esize = 4;  // bytes per element
    size_t qes = 4;    // bytes per stored forward-term element
    // checkpointing (SURVEY s.8f-3): snapshot of (u^n, u^{n-1}) every `ckpt` steps instead of the
    // imaging term of every step; q_store then holds ckpt + 1 slots and fwd[] the recomputed fields
    int ckpt = 0;
    int istride = 1;     // imaging stride: the forward term is stored / correlated every istride-th step
    bool inc = false;    // increment form: state (u, v = u - u_prev); u[] ping-pongs u, v lives in vf
    bool cpml = false;   // convolutional PML (abc = FWI_ABC_CPML with npml > 0)
    bool qbf16 = false;  // forward-term store in bf16 (fp32 3-D stream contexts)
    // 2-D temporal blocking (fwi_fused2d.hip)
    bool fused2d = false;
    int fused_ft = FUSED2D_TILE;  // interior tile edge of the fused 2-D kernel (fused2d_pick_tile; 64 with CPML / increment)
    int fused_skipd = -1;         // Fused2dArgs::skipd (Hooks::fused_skipd)
    // 3-D temporal blocking (fwi_pair3d.hip): forward sweeps without imaging advance two steps per pass
    bool pair3d = false;
    int pair_zc = 0, pair_tw = 256;
    int pml_lines = 0;  // axes (z = 1, y = 2) whose border runs as one line launch per step (pml_line_axes)
    bool xpml = false;  // 3-D fp32 stream contexts: the x border's recursion runs inside the step kernel
    // Placement of the small arrays the 3-D step kernel streams beside the fields, each inside an allocation `place_pad`
    // bytes longer than the array.  place_kind 1, contexts with the x border in the kernel: the handed-over terms ty and
    // tz, the x border's zeta and psi (and v in increment form); 2, increment-form contexts without CPML: v and C --
    // worth 1.5 - 3 % there, the per-process spread of that form is not theirs to fix; the u buffers change roles with
    // others and stay put.  place_mode: where in the pad they go -- nowhere (PAD), where Impl::tune_placement measures
    // the step as fastest (SEARCH), or fixed_k[i] x 2 MiB for movable array i in the search order (FIXED).
    int place_kind = 0;
    size_t place_pad = 0;
    PlaceMode place_mode = PLACE_OFF;
    int fixed_k[8] = {};
};

// The plan of a configuration that has passed fwi_create's argument checks.  FWI_OK, or FWI_EINVAL with the reason in
// *why (fwi_create puts "fwi_create: " before it): a stream kernel that does not exist for the configuration -- nothing
// of *plan is decided then -- or a malformed "fixed:" on a context that places, which is found last: *plan is complete
// and place_kind says what would have been placed.
int plan_context(const fwi_config &cfg, const Hooks &hooks, Plan *plan, std::string *why);
// The context's own statement of its path (FWI_DEBUG_PML), without a newline
void plan_report(const Plan &plan, char *buf, size_t len);
const char *plan_kernel_name(const Plan &plan);

}  // namespace fwi
