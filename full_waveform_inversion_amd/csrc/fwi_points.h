// A shot's point tables: which amplitudes each workgroup of each step kernel injects and which cells it samples, built
// from the plan and the caller's grid indices alone.  Plain C++ (no HIP, no device, no dtype): Impl<T>::upload_set and
// set_spread (fwi_api.hip) permute the typed coefficients by a table's `col` and upload; tests/points_host.cpp builds the
// same tables on the CPU.  Every table must agree with its kernel's block decode -- each function names the kernel.
#pragma once
#include <stdint.h>

#include <vector>

#include "fwi_plan.h"

namespace fwi {

// (n, ndim) int32 grid indices -> padded / compact flat indices
struct FlatPoints {
    std::vector<int64_t> pidx, cidx;
};
// Returns the first point outside the grid (the indices up to it are filled in), or -1
int flatten(const GridDesc &g, const int32_t *idx, int n, FlatPoints *out);

// Workgroup tile of the stream kernel that owns grid point (z, y, x): the index into StepArgs::inj_start.  Must match
// the block decode of step3d_stream (fwi_stream3d.h) in 3-D and of step2d_tile (fwi_kernels.hip) in 2-D.
int stream_tile_of(const GridDesc &g, const StreamTuning &t, int z, int y, int x);
int stream_num_tiles(const GridDesc &g, const StreamTuning &t);
// Same for the point kernel (64 x 4 point workgroups): step_point's block decode, launch_point_mode's point_blocks
// (fwi_kernels.hip).
int point_tile_of(const GridDesc &g, int z, int y, int x);
int point_num_tiles(const GridDesc &g);

// The set sorted by the step kernel's workgroup tile (Plan::kernel), within a tile by node, then by entry: the entries of
// one node are consecutive, and the kernels add such a run from one thread in this order (inject_runs).
struct StepTable {
    std::vector<int> start;          // tiles + 1: CSR over the tiles
    std::vector<int64_t> pidx, cidx;
    std::vector<int> col;            // the point an entry came from
    std::vector<int> run;            // run length at the first entry of each node's run, 0 at the others
};
void step_table(const Plan &plan, const int32_t *idx, int n, const FlatPoints &flat, StepTable *out);

// Entries of the fused 2-D kernel (step2d_fused, Plan::fused2d): a point is injected by every tile whose EXTENDED region
// holds it (each keeps a private copy of the halo) and sampled by the one tile that owns it.  With the CPML inside the
// launch the tiles are whole, with one overlap seam per axis (fused2d_origin / fused2d_own).
struct Fused2dTables {
    // injection: CSR over the tiles, sorted within a tile by node, then by entry
    std::vector<int> start, lz, lx;  // (lz, lx): the cell within the tile's extended region
    std::vector<int> col;
    std::vector<unsigned char> interior;  // the tile owns the point
    std::vector<int> run;                 // as StepTable::run, per (tile, node)
    // sampling: the interior entries alone, in the same order
    std::vector<int> rstart, rlz, rlx, rcol;
};
void fused2d_tables(const Plan &plan, const int32_t *idx, int n, Fused2dTables *out);

// Entries of the two-step 3-D kernel (step3d_pair, Plan::pair3d), CSR over its workgroups in the kernel's renumbered
// order: a point is injected by every workgroup whose step-1 region (tile widened by r) holds it.  Pair3dInj::cu is left
// 0 for the caller (cu[col]).
struct Pair3dTable {
    std::vector<int> start;
    std::vector<Pair3dInj> ent;
};
void pair3d_table(const Plan &plan, const int32_t *idx, int n, Pair3dTable *out);

// Off-grid points (fwi_forward_spread): nodes of point p = entries pt_start[p] .. pt_start[p + 1] of the node list, at
// most 8.  owner[m] is the point of entry m.  `check` says which requirement the set misses (the first one, in this order).
enum SpreadCheck {
    SPREAD_OK = 0,
    SPREAD_BAD_SET,               // npts < 0, or points without pt_start or weights
    SPREAD_NODES_WITHOUT_POINTS,  // npts == 0 but nnodes != 0
    SPREAD_BAD_RANGE,             // pt_start does not run from 0 to nnodes
    SPREAD_BAD_COUNT,             // `point` has `count` nodes, outside 0 .. 8
};
struct SpreadOwners {
    SpreadCheck check = SPREAD_OK;
    int point = -1, count = 0;
    std::vector<int> owner;
};
SpreadOwners spread_owners(int npts, int nnodes, const int32_t *pt_start, bool have_weight);

}  // namespace fwi
