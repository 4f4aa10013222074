"""What a shot's point tables must hold, restated from the definitions (tests/test_points_host.py holds csrc/fwi_points.cpp
to it, exactly).  Nothing here searches or counts the way the C++ does: a point's tiles are found by asking EVERY tile
whether its region holds the point, and entries are put in order by sorting on the key the kernels rely on -- tile, then
node, then entry order -- with the run length at the first entry of each (tile, node) run and 0 at the others.

``plan`` is what tests/points_host.cpp prints of the plan (launch shape, tile edge, seam, strides); ``shape`` is (nz, nx) or
(nz, ny, nx); ``pts`` a list of index tuples in the caller's order."""
import itertools

HALO = 4            # fwi_plan.h
FUSED2D_STEPS = 4
PAIR3D_TY = 8
K_POINT, K_STREAM = 1, 2


def zyx(shape, p):
    return (p[0], p[1], p[2]) if len(shape) == 3 else (p[0], 0, p[1])


def dims(shape):
    return (shape[0], shape[1], shape[2]) if len(shape) == 3 else (shape[0], 1, shape[1])


def flatten(plan, shape, pts):
    """(first point outside the grid or -1, padded indices, compact indices)"""
    nz, ny, nx = dims(shape)
    pidx, cidx = [], []
    for i, p in enumerate(pts):
        z, y, x = zyx(shape, p)
        if not (0 <= z < nz and 0 <= y < ny and 0 <= x < nx):
            return i, None, None
        pidx.append(plan["off0"] + z * plan["sz"] + y * plan["sy"] + x)
        cidx.append((z * ny + y) * plan["cx"] + x)
    return -1, pidx, cidx


def blocks(n, size):
    """[lo, hi) of the blocks of ``size`` cells that cover an axis of n cells"""
    return [(lo, min(lo + size, n)) for lo in range(0, n, size)]


def inside(box, q):
    return all(lo <= c < hi for (lo, hi), c in zip(box, q))


def csr(tiles, ntile):
    start = [0] * (ntile + 1)
    for t in tiles:
        start[t + 1] += 1
    for t in range(ntile):
        start[t + 1] += start[t]
    return start


def runs(keys):
    """Length of each run of equal consecutive keys at its first entry, 0 at the others"""
    out = []
    for _, grp in itertools.groupby(keys):
        k = len(list(grp))
        out += [k] + [0] * (k - 1)
    return out


def step_boxes(plan, shape):
    """The cells each workgroup of the step kernel writes, in workgroup order (x tiles fastest, then rows, then planes or
    chunks of planes): the stream kernel marches zchunk planes over ty rows of y (2-D: the tile kernel takes ty rows of z);
    the point kernel takes 64 columns x 4 rows, of one plane in 3-D."""
    nz, ny, nx = dims(shape)
    if plan["kernel"] == K_STREAM:
        per = (plan["zchunk"], plan["ty"], plan["tile_x"]) if len(shape) == 3 else (plan["ty"], 1, plan["tile_x"])
    else:
        per = (1, 4, 64) if len(shape) == 3 else (4, 1, 64)
    return list(itertools.product(blocks(nz, per[0]), blocks(ny, per[1]), blocks(nx, per[2])))


def step_table(plan, shape, pts):
    _, pidx, cidx = flatten(plan, shape, pts)
    boxes = step_boxes(plan, shape)
    ents = []
    for i, p in enumerate(pts):
        owners = [t for t, box in enumerate(boxes) if inside(box, zyx(shape, p))]
        assert len(owners) == 1, (p, owners)    # the workgroups' cells partition the grid
        ents.append((owners[0], pidx[i], i))
    ents.sort()
    return {"step.start": csr([e[0] for e in ents], len(boxes)), "step.pidx": [e[1] for e in ents],
            "step.cidx": [cidx[e[2]] for e in ents], "step.col": [e[2] for e in ents], "step.run": runs([e[:2] for e in ents])}


def fused2d_origin(t, n, ft, seam):
    """First cell of tile t of an axis of n cells.  Plain tiling: t * ft.  With the seam (CPML inside the launch) the tiles
    are whole: the lower half of them starts at t * ft, the upper half is anchored at the high end of the axis, origins
    rounded up to a multiple of 4."""
    nt = -(-n // ft)
    if not seam or nt < 2 or t < nt // 2:
        return t * ft
    return -(-(n - (nt - t) * ft) // 4) * 4


def fused2d_axis(n, ft, seam, hl):
    """Per tile of the axis: (extended region, owned cells).  A tile owns from where the tile below it ends."""
    nt = -(-n // ft)
    org = [fused2d_origin(t, n, ft, seam) for t in range(nt)]
    own = [0] + [o + ft for o in org[:-1]] + [n]
    return [((org[t] - hl, org[t] + ft + hl), (own[t], own[t + 1])) for t in range(nt)]


def fused2d_halo(plan):
    return (FUSED2D_STEPS * plan["r"] + 3) // 4 * 4


def fused2d_tables(plan, shape, pts):
    ft, seam, hl = plan["fused_ft"], plan["cpml"], fused2d_halo(plan)
    az, ax = fused2d_axis(shape[0], ft, seam, hl), fused2d_axis(shape[1], ft, seam, hl)
    ents = []
    for (tz, (ez, oz)), (tx, (ex, ox)) in itertools.product(enumerate(az), enumerate(ax)):
        for i, (z, x) in enumerate(pts):
            if inside((ez, ex), (z, x)):
                ents.append((tz * len(ax) + tx, z - ez[0], x - ex[0], i, int(inside((oz, ox), (z, x)))))
    ents.sort(key=lambda e: e[:4])      # tile, node (lz, lx), entry
    own = [e for e in ents if e[4]]
    ntile = len(az) * len(ax)
    return {"fused.start": csr([e[0] for e in ents], ntile), "fused.lz": [e[1] for e in ents], "fused.lx": [e[2] for e in ents],
            "fused.col": [e[3] for e in ents], "fused.interior": [e[4] for e in ents], "fused.run": runs([e[:3] for e in ents]),
            "fused.rstart": csr([e[0] for e in own], ntile), "fused.rlz": [e[1] for e in own], "fused.rlx": [e[2] for e in own],
            "fused.rcol": [e[3] for e in own]}


def pair3d_boxes(plan, shape):
    """Per workgroup of the two-step kernel, x tiles fastest: (its own cells, the column of lane 0).  Rows of at most 256
    columns are one tile that starts at column 0; wider rows are cut into tiles of pair_tw columns, whose lane 0 sits two
    halos left of the tile."""
    nz, ny, nx = shape
    bx = [(0, nx)] if nx <= 256 else blocks(nx, plan["pair_tw"])
    # (the last row tile is PAIR3D_TY rows whatever ny: the rows past the grid hold no point)
    by = [(lo, lo + PAIR3D_TY) for lo in range(0, ny, PAIR3D_TY)]
    return [((z, y, x), 0 if len(bx) == 1 else x[0] - 2 * HALO)
            for z, y, x in itertools.product(blocks(nz, plan["pair_zc"]), by, bx)]


def pair3d_table(plan, shape, pts):
    r, boxes = plan["r"], pair3d_boxes(plan, shape)
    one = len(boxes) and boxes[0][0][2] == (0, shape[2])
    ents = []
    for t, (box, xbase) in enumerate(boxes):
        # step 1 computes the tile widened by r; a row that is one tile holds every column
        wide = tuple((lo - r, hi + r) for lo, hi in box[:2]) + ((box[2] if one else (box[2][0] - r, box[2][1] + r)),)
        for i, p in enumerate(pts):
            if inside(wide, p):
                ents.append((t, i, [p[0], p[1] - box[1][0], p[2] - xbase, i, int(inside(box, p))]))
    ents.sort(key=lambda e: e[:2])      # workgroup, then entry order
    return {"pair.start": csr([e[0] for e in ents], len(boxes)), "pair.ent": [v for e in ents for v in e[2]]}


SPREAD_OK, SPREAD_BAD_SET, SPREAD_NODES_WITHOUT_POINTS, SPREAD_BAD_RANGE, SPREAD_BAD_COUNT = range(5)


def spread_owners(npts, nnodes, pt_start, have_weight):
    """(check, point, count, owners): the first requirement an off-grid point set misses (include/fwi.h,
    fwi_forward_spread), or the point each node entry belongs to."""
    if npts < 0 or (npts > 0 and (pt_start is None or not have_weight)):
        return SPREAD_BAD_SET, -1, 0, []
    if npts == 0:
        return (SPREAD_NODES_WITHOUT_POINTS if nnodes else SPREAD_OK), -1, 0, []
    if pt_start[0] != 0 or pt_start[npts] != nnodes:
        return SPREAD_BAD_RANGE, -1, 0, []
    counts = [b - a for a, b in zip(pt_start[:npts], pt_start[1:npts + 1])]
    for p, k in enumerate(counts):
        if not 0 <= k <= 8:
            return SPREAD_BAD_COUNT, p, k, []
    return SPREAD_OK, -1, 0, [p for p, k in enumerate(counts) for _ in range(k)]
