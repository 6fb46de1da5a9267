"""TEST-ONLY scene builders and checkers for the neighbour build (cell keys, stable radix sort, reorder, cell-range table and its two
queued-ahead forms): tests/test_neighbour_build_scenes.py proves on the CPU what every scene exercises and that the checkers bite,
tests/test_gpu_neighbour_build.py runs the scenes on the device against the oracle.  Nothing in the product package imports this.

The size of the cell grid is the bounding box, not the particle count: a few small clumps far apart reach every digit plan of the sort,
every branch of the cell-range table and the limits of the grid with a few hundred particles."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

from adaptive_sph_amd import scene as sc

REPO = Path(__file__).resolve().parent.parent

# adaptive_sph_amd/csrc/sph_sort.hip, restated (test_the_constants_restated_here_are_the_products reads them from the source)
RS_TILE = 2048            # keys per workgroup of a sort pass: 64 x RS_ITEMS
RS_TRIP = 1024            # tiles one trip of k_rs_rowscan scans: 256 threads x 4 counts
CS_INLINE = 64            # a gap of >= 64 cells between two occupied keys goes to the work list ...
CS_WORK_CAP = 65536       # ... unless the list is full: then the owning thread fills it after all
MERGE_SLACK = 4096        # the merge is admitted for a predicted grid of at most n + 4096 cells (sph_grid_plan.hpp: inc_sort_fits)
AHEAD_MARGIN = 2          # cells the predicted grid of a uniform scene adds on every side
GRID_DIM_LIMIT = 65536    # a grid dimension must stay below it (cx | cy << 16), the cell count below 2^27
GRID_CELL_LIMIT = 1 << 27

D = 1.0 / 64.0            # rest spacing of the clumps


def product_constants():
    """the #defines of sph_sort.hip the figures above restate"""
    text = (REPO / "adaptive_sph_amd" / "csrc" / "sph_sort.hip").read_text()
    val = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", text).group(1))
    return dict(RS_TILE=64 * val("RS_ITEMS"), CS_INLINE=val("CS_INLINE"), CS_WORK_CAP=val("CS_WORK_CAP"))


def h_of_mass(mass, rest_density=1.0):
    """h_next_from_mass in f32: 1.9 sqrt((m / rho0) (1 / pi))"""
    vol = np.asarray(mass, np.float32) / np.float32(rest_density)
    return np.float32(1.9) * np.sqrt(vol * np.float32(0.318309873342514038086), dtype=np.float32)


def ilog2_ceil(v):
    b = 0
    while (1 << b) < int(v):
        b += 1
    return b


def digit_plan(ncells):
    """(passes, digit width) radix_sort_pairs takes for keys below `ncells`: the fewest passes of at most 10 bits, then the narrowest
    digit of at least 8 bits that covers the key in that many"""
    bits = max(ilog2_ceil(ncells), 1)
    passes = (bits + 9) // 10
    return passes, max((bits + passes - 1) // passes, 8)


ALL_PLANS = [(1, 8), (1, 9), (1, 10), (2, 8), (2, 9), (2, 10), (3, 8), (3, 9)]


def box_planes(pos, pad=8.0):
    """an AnalyticOverestimate box about the origin that holds `pos` with `pad` to spare: no particle is near a wall"""
    w = 2.0 * (float(np.abs(pos[:, 0]).max()) + pad)
    hgt = 2.0 * (float(np.abs(pos[:, 1]).max()) + pad)
    return sc.boundary_planes(sc.SceneBoundary("box", w, hgt))


def sparse_sites(sites, k=3, d=D, fill=1.0):
    """Clumps of k x k equal particles (k = 3 or 4) at rest spacing `d`, one per site; a site (ix, iy) is the CORNER between the cells
    ix - 1 | ix and iy - 1 | iy of the grid whose cell is the particles' support 2 h.  A clump straddles its corner: particles in four
    cells, each with neighbours in another cell.  (k = 3: moved d / 4 off the corner, so that no particle sits ON a cell boundary.)
    Sites at least 4 cells apart along an axis leave two empty cells between clumps: every neighbour of a particle lies in its own clump.
    The occupied cells are ix - 1 .. ix, so the reported grid (one empty cell on every side of the occupied ones) has
        size_x = max ix - min ix + 4,  size_y = max iy - min iy + 4.
    Returns a scene dict: mass, pos, vel, planes, clump (the site of every particle), k."""
    sites = np.asarray(sites, np.int64).reshape(-1, 2)
    assert k in (3, 4) and len(sites)
    mass1 = np.float32(d) * np.float32(d) * np.float32(fill)
    cs = float(np.float32(2.0) * h_of_mass(mass1))
    # centred about the origin: the coordinates (hence their f32 spacing) stay as small as the extent allows
    mid = (sites.min(axis=0) + sites.max(axis=0)) // 2
    off = (np.arange(k, dtype=np.float64) - (k - 1) / 2.0) * d + (0.25 * d if k == 3 else 0.0)
    ox, oy = np.meshgrid(off, off, indexing="ij")
    centre = (sites - mid).astype(np.float64) * cs
    pos = np.empty((len(sites), k * k, 2), np.float64)
    pos[:, :, 0] = centre[:, 0, None] + ox.reshape(-1)[None, :]
    pos[:, :, 1] = centre[:, 1, None] + oy.reshape(-1)[None, :]
    pos = pos.reshape(-1, 2).astype(np.float32)
    n = len(pos)
    return dict(mass=np.full(n, mass1, np.float32), pos=pos, vel=np.zeros((n, 2), np.float32), planes=box_planes(pos),
                clump=np.repeat(np.arange(len(sites)), k * k), k=k, cell_size=cs, sites=sites)


def shuffled(scene, seed=1234):
    """the same particles in a fixed-seed random upload order"""
    perm = np.random.default_rng(seed).permutation(len(scene["mass"]))
    out = dict(scene)
    for key in ("mass", "pos", "vel", "clump"):
        if scene.get(key) is not None:
            out[key] = np.ascontiguousarray(scene[key][perm])
    return out


def corner_sites(sx, sy, count=60, seed=0, pitch=4):
    """sites for a grid of exactly sx x sy cells: the two opposite corners of the site range and up to `count` more on a lattice of
    `pitch` cells in between (fixed seed)"""
    wx, wy = sx - 4, sy - 4
    assert wx >= 0 and wy >= 0
    gx, gy = np.arange(0, wx + 1, pitch), np.arange(0, wy + 1, pitch)
    # (the far corner may lie off the lattice: lattice points closer than `pitch` to it are left out)
    gx, gy = gx[(wx - gx >= pitch) | (gx == wx)], gy[(wy - gy >= pitch) | (gy == wy)]
    rng = np.random.default_rng(seed)
    total = len(gx) * len(gy)
    if total <= count:
        ix, iy = np.meshgrid(gx, gy, indexing="ij")
        pick = np.stack([ix.reshape(-1), iy.reshape(-1)], axis=1)
    else:
        flat = rng.choice(total, count, replace=False)
        pick = np.stack([gx[flat // len(gy)], gy[flat % len(gy)]], axis=1)
    far = np.array([[wx, wy]])
    near_far = (np.abs(pick[:, 0] - wx) < pitch) & (np.abs(pick[:, 1] - wy) < pitch)
    pick = pick[~near_far]
    sites = np.unique(np.concatenate([[[0, 0]], pick, far]), axis=0)
    return sites


def row_sites(pitches, n_rows, row_pitch=4, width=None):
    """site rows `row_pitch` cells apart; row r repeats the x pitch pitches[r % len(pitches)] from 0 while the site stays below `width`
    (default: 12 sites per row).  Two sites `p` cells apart leave p - 2 empty cells between their clumps."""
    out = []
    for r in range(n_rows):
        p = pitches[r % len(pitches)]
        m = 12 if width is None else (width - 4) // p + 1
        out.append(np.stack([np.arange(m) * p, np.full(m, r * row_pitch)], axis=1))
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------
# the reference of the neighbour sets, independent of any grid
# ------------------------------------------------------------------------------------------------
def csr_keys(offsets, indices):
    """(row << 32 | index) of every CSR entry, sorted: two lists hold the same SETS iff the arrays are equal"""
    off = np.asarray(offsets).astype(np.int64)
    rows = np.repeat(np.arange(len(off) - 1, dtype=np.uint64), np.diff(off)) << np.uint64(32)
    keys = rows | np.asarray(indices).astype(np.uint64)
    keys.sort()
    return keys


def brute_force_keys(scene):
    """csr_keys of the neighbour sets by brute force, dense numpy, the reference's predicate in f32 with its operations:
    dx * dx + dy * dy < s * s,  s = ((h_i + h_j) * 0.5) * 2  (every particle is on its own list).  A sparse-site scene clump by clump
    (every neighbour lies in the particle's own clump: clumps_are_apart); any other scene of a few thousand particles all pairs."""
    if scene.get("clump") is None:
        assert len(scene["mass"]) <= 4096
        ids = np.arange(len(scene["mass"]))[None, :]
    else:
        order = np.argsort(scene["clump"], kind="stable")      # particle ids clump by clump (any upload order)
        ids = order.reshape(-1, scene["k"] ** 2)
    x = scene["pos"][ids].astype(np.float32)                   # (clumps, particles of one, 2)
    h = h_of_mass(scene["mass"])[ids]
    dx = x[:, :, None, 0] - x[:, None, :, 0]
    dy = x[:, :, None, 1] - x[:, None, :, 1]
    r2 = dx * dx + dy * dy
    s = ((h[:, :, None] + h[:, None, :]) * np.float32(0.5)) * np.float32(2.0)
    assert r2.dtype == np.float32 and s.dtype == np.float32
    c, i, j = np.nonzero(r2 < s * s)
    keys = (ids[c, i].astype(np.uint64) << np.uint64(32)) | ids[c, j].astype(np.uint64)
    keys.sort()
    return keys


def clumps_are_apart(scene):
    """no two clumps share or touch a cell, with a cell to spare: the 4 x 4 cells around every site (its clump's four and one on every
    side) belong to that site alone"""
    sites = scene["sites"]
    r = np.arange(-2, 2)
    cx = (sites[:, 0, None, None] + r[None, :, None]) + 0 * r[None, None, :]
    cy = (sites[:, 1, None, None] + r[None, None, :]) + 0 * r[None, :, None]
    keys = (cx.reshape(-1) + (1 << 20)) * (1 << 22) + (cy.reshape(-1) + (1 << 20))
    return len(np.unique(keys)) == 16 * len(sites)


# ------------------------------------------------------------------------------------------------
# the order check, the key gaps, and a numpy model of the device's build to show that the checks bite
# ------------------------------------------------------------------------------------------------
def slot_order_violations(offsets, indices, cell_index):
    """The device visits a particle's neighbours in ascending SLOT of its cell-sorted array (rows of cells bottom to top, slots ascending
    inside a row) and exports them in that order; on the first step after an upload the slot of host particle i is its rank in the stable
    sort by cell (oracle_harness.device_slots; the same order as test_gpu_bitexact.device_order: lexsort by (cy, cx), ties in upload
    order).  Number of adjacent entries of a row that are NOT strictly ascending in that predicted slot: 0 for a stable sort."""
    from tests.oracle_harness import device_slots
    slot = device_slots(cell_index)
    off = np.asarray(offsets).astype(np.int64)
    s = slot[np.asarray(indices).astype(np.int64)]
    bad = np.diff(s) <= 0
    bad[off[1:-1] - 1] = False          # the step from one row to the next
    return int(bad.sum())


def key_gaps(cell_index):
    """b - a - 1 for consecutive distinct occupied keys a < b: the empty cells k_cell_start fills between them (>= 64: work list)"""
    keys = np.unique(np.asarray(cell_index).astype(np.int64))
    return np.diff(keys) - 1


def cell_table(cell_index, ncells):
    """the exclusive cell-range table: cell_start[c] = number of particles in cells < c, [ncells] = n"""
    return np.concatenate([[0], np.cumsum(np.bincount(np.asarray(cell_index).astype(np.int64), minlength=ncells))]).astype(np.int64)


def model_device_lists(scene, grid, cell_index, perm=None, table=None):
    """What the device's build gives for a ONE-SIZE scene, in numpy: `perm` (slot -> host particle; default the stable sort by cell) and
    `table` (default cell_table) as the sort and k_cell_start leave them, then every particle's walk over its 3 x 3 cells through the table
    with the predicate of brute_force_keys, the hits exported as host ids in slot order.  Returns CSR (offsets, indices) in host order."""
    sx, sy = int(grid.size_x), int(grid.size_y)
    ci = np.asarray(cell_index).astype(np.int64)
    n = len(ci)
    if perm is None:
        perm = np.argsort(ci, kind="stable")
    if table is None:
        table = cell_table(ci, sx * sy)
    x = scene["pos"][perm].astype(np.float32)
    h = h_of_mass(scene["mass"])[perm]
    key = ci[perm]
    rows = [None] * n
    for i in range(n):
        cx, cy = int(key[i] % sx), int(key[i] // sx)
        out = []
        for yy in range(cy - 1, cy + 2):
            if yy < 0 or yy >= sy:
                continue
            b, e = int(table[yy * sx + max(cx - 1, 0)]), int(table[yy * sx + min(cx + 2, sx)])
            if e <= b:
                continue
            j = np.arange(b, min(e, n))
            dx, dy = x[i, 0] - x[j, 0], x[i, 1] - x[j, 1]
            s = ((h[i] + h[j]) * np.float32(0.5)) * np.float32(2.0)
            out.append(perm[j[dx * dx + dy * dy < s * s]])
        rows[int(perm[i])] = np.concatenate(out) if out else np.zeros(0, np.int64)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    return offsets, np.concatenate(rows).astype(np.uint32)


# ------------------------------------------------------------------------------------------------
# the scenes
# ------------------------------------------------------------------------------------------------
# a. one scene per end of every digit plan's bit range: name -> (size_x, size_y); the grid the product sorts the FIRST build by
PLAN_GRIDS = {
    "bits04_one_clump": (4, 4),            # (1, 8)  the smallest grid there is; n = 16 < 64: not one full wave
    "bits08_2pow8": (16, 16),              # (1, 8)  last
    "bits09": (20, 24),                    # (1, 9)
    "bits10_2pow10": (32, 32),             # (1, 10) exactly 2^10 cells
    "bits11_2pow10_plus_row": (32, 33),    # (2, 8)  first: 2^10 and one row
    "bits16_2pow16": (256, 256),           # (2, 8)  last
    "bits17": (256, 257),                  # (2, 9)  first
    "bits18_2pow18": (512, 512),           # (2, 9)  last
    "bits19": (512, 516),                  # (2, 10) first
    "bits20_2pow20": (1024, 1024),         # (2, 10) last: exactly 2^20 cells
    "bits21_above_2pow20": (1025, 1025),   # (3, 8)  first
    "bits24_2pow24": (4096, 4096),         # (3, 8)  last: exactly 2^24 cells, a 67 MB table
    "bits25_above_2pow24": (4104, 4104),   # (3, 9)  first -- its last bit count, 27, is the grid limit itself: not approached
}


def plan_scene(name):
    sx, sy = PLAN_GRIDS[name]
    return sparse_sites(corner_sites(sx, sy, count=120, seed=sx * 31 + sy), k=4 if name == "bits04_one_clump" else 3)


def dense_block(nx, ny, spacing=1.0 / 64, cut=None):
    """dam_break_small's lattice (x outer, y inner); `cut`: only the first `cut` particles -- whole columns and one cut short"""
    scn = sc.dam_break_small(nx, ny, spacing)
    pos, mass, vel = sc.init_particles(scn)
    if cut is not None:
        pos, mass, vel = pos[:cut].copy(), mass[:cut].copy(), vel[:cut].copy()
    return dict(mass=mass, pos=pos, vel=vel, planes=sc.boundary_planes(scn.boundary), clump=None, k=None)


# c. tile and trip edges: n -> a lattice of `rows` particles per column with the last column cut
EDGE_COUNTS = {63: 8, 64: 8, 65: 8, 1023: 32, 1024: 32, 1025: 32, 2047: 32, 2048: 32, 2049: 32}


def edge_scene(n):
    rows = EDGE_COUNTS[n]
    return dense_block((n + rows - 1) // rows, rows, 1.0 / 64, cut=n)


def big_lattice(side):
    """side x side particles at spacing 1/1024 (dam_break_1m's) in a box that holds them"""
    s = 1.0 / 1024
    width = 2.0 * np.ceil(side * s / 2.0 + 1.0)
    scn = sc.SceneConfig(sc.SceneBoundary("box", float(width), 4.0),
                         [sc.SceneFluidBlock([-width / 2 + 0.001, -1.999], [side * s + 0.5 * s, side * s + 0.5 * s], s, 0.93, [0.0, 0.0])])
    pos, mass, vel = sc.init_particles(scn)
    assert len(mass) == side * side
    return dict(mass=mass, pos=pos, vel=vel, planes=sc.boundary_planes(scn.boundary), clump=None, k=None)


# d. the cell table
def table_threshold_scene():
    """rows of sites at pitch 65 and at pitch 66: 63 and 64 empty cells between consecutive clumps, either side of CS_INLINE"""
    return sparse_sites(row_sites([65, 66, 67, 66, 65], 10), k=3)


def table_overflow_scene():
    """990 sites per row at pitch 66 (64 empty cells between clumps: a work-list entry each, twice per site row), 36 site rows: more
    entries than the work list holds, so k_cell_start falls back to the inline loop for the rest; size_x = 65 278"""
    return sparse_sites(row_sites([66], 36, row_pitch=4, width=65282), k=3)


# e. grid limits
def strip_sites(length, rows=2, count=150, seed=5):
    """sites on `rows` rows 4 cells apart between x = 0 and x = length - 4 (size_x = length)"""
    rng = np.random.default_rng(seed)
    xs = np.unique(np.concatenate([[0, length - 4], rng.integers(1, (length - 8) // 4, count) * 4]))
    return np.stack([xs, (np.arange(len(xs)) % rows) * 4], axis=1)


def limit_scene(length, transpose=False):
    sites = strip_sites(length)
    s = sparse_sites(sites[:, ::-1] if transpose else sites, k=3)
    return s


LIMIT_FITS, LIMIT_REFUSED = 65532, 65540     # size along the strip: below 65 536 (a full 16-bit cell coordinate) and past it


# f. multi-resolution strips
def two_size_strip(extent, ratio, d_fine=D, fill=0.93):
    """a fine block at x = -extent / 2; at x = +extent / 2 a coarse block (`ratio` x the spacing) with a second fine block standing
    against its left side, one mean spacing away: fine and coarse particles on each other's lists from step 0"""
    dc = d_fine * ratio

    def lattice(x0, y0, nx, ny, d):
        ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
        p = np.stack([x0 + ix.reshape(-1) * d, y0 + iy.reshape(-1) * d], axis=1)
        return p, np.full(len(p), np.float32(d) * np.float32(d) * np.float32(fill), np.float32)

    parts = [lattice(-extent / 2, 0.0, 12, 12, d_fine),
             lattice(extent / 2, 0.0, 5, 5, dc),
             lattice(extent / 2 - 0.5 * (d_fine + dc) - 9 * d_fine, 0.0, 10, 14, d_fine)]
    pos = np.concatenate([p for p, _ in parts]).astype(np.float32)
    mass = np.concatenate([m for _, m in parts])
    return dict(mass=mass, pos=pos, vel=np.zeros_like(pos), planes=box_planes(pos), clump=None, k=None)


MULTIRES_SCENES = {
    # name -> (extent, size ratio, cell doublings the product takes, tile side in sorting cells)
    "fine_grid_fits": (6.0, 4, 0, 4),
    "cell_doubled_once": (2600.0, 4, 1, 2),       # ~80 000 fine cells wide: the fine grid does not fit, twice its cell does
    "coarse_grid_only": (2600.0, 2, None, 1),     # size ratio 2: twice the fine cell IS the coarse cell -- the tile_ts = 1 fallback
}


def sorting_grid(pos, mass):
    """plan_grid and plan_sorting_grid (csrc/sph_grid_plan.hpp: the coarse grid and the search for the sorting grid of a multi-resolution
    scene) restated in f32 like the product -- tests/test_build_plan_host.py compares the two on the CPU:
    -> (coarse (sx, sy), sorting (sx, sy), doublings or None for the fallback, tile side)"""
    h = h_of_mass(mass)
    lo, hi = pos.min(axis=0).astype(np.float32), pos.max(axis=0).astype(np.float32)

    def make_grid(cs):
        cs = np.float32(cs)
        mn = np.floor(lo / cs).astype(np.int64) - 1
        sz = np.floor(hi / cs).astype(np.int64) + 2 - mn
        ok = (sz > 0).all() and (sz < GRID_DIM_LIMIT).all() and int(sz[0]) * int(sz[1]) < GRID_CELL_LIMIT
        return ok, (int(sz[0]), int(sz[1]))

    gcs = np.float32(h.max() * np.float32(2.0))
    ok, coarse = make_grid(gcs)
    assert ok
    if not (h.max() >= np.float32(1.75) * h.min()):
        return coarse, coarse, 0, 0
    cs = np.float32(h.min() * np.float32(2.0))
    k = 0
    while k < 24 and cs < gcs:
        ok, fine = make_grid(cs)
        if ok:
            ts = int(np.ceil(gcs / cs))
            while np.float32(ts) * cs < gcs:
                ts += 1
            return coarse, fine, k, ts
        k, cs = k + 1, np.float32(cs * np.float32(2.0))
    return coarse, coarse, None, 1


# g. the merge at its admission limit
def two_blocks(gap_cells, side=32, d=D, speed=0.5):
    """two side x side blocks moving towards each other along x at `speed`, `gap_cells` cells of empty grid between them; their outer
    edges stand in the middle of a cell, so the few steps of the test move no edge over a cell boundary"""
    mass1 = np.float32(d) * np.float32(d) * np.float32(0.93)
    cs = float(np.float32(2.0) * h_of_mass(mass1))
    ix, iy = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    lat = np.stack([ix.reshape(-1) * d, iy.reshape(-1) * d], axis=1)
    width_cells = int(np.ceil((side - 1) * d / cs)) + 1
    left = lat + np.array([0.5 * cs, 0.5 * cs])
    right = lat + np.array([(width_cells + gap_cells + 0.5) * cs, 0.5 * cs])
    pos = np.concatenate([left, right])
    pos -= 0.5 * (pos.min(axis=0) + pos.max(axis=0))
    # (after centring: keep the edges in mid-cell)
    pos += (0.5 - np.mod(pos.min(axis=0) / cs, 1.0)) * cs
    vel = np.zeros_like(pos)
    vel[: side * side, 0], vel[side * side:, 0] = speed, -speed
    pos = pos.astype(np.float32)
    return dict(mass=np.full(len(pos), mass1, np.float32), pos=pos, vel=vel.astype(np.float32), planes=box_planes(pos), clump=None, k=None)


def merge_gap_for(side=32, admitted=True):
    """the gap (cells) at which the PREDICTED grid of the two blocks -- the reported one plus 2 cells on every side -- holds at most
    (`admitted`) / more than n + 4096 cells, as close to that limit as whole columns allow"""
    n = 2 * side * side
    g = 0
    while True:
        s = two_blocks(g, side)
        (sx, sy), _, _, _ = sorting_grid(s["pos"], s["mass"])
        if (sx + 2 * AHEAD_MARGIN) * (sy + 2 * AHEAD_MARGIN) > n + MERGE_SLACK:
            return g - 1 if admitted else g + (0 if sx * sy > n + MERGE_SLACK else int(np.ceil((n + MERGE_SLACK + 1 - sx * sy) / sy)))
        g += 1


def forced_params(**kw):
    """the dam break's parameters with the iteration counts forced (tolerances 0): both sides run max_iters iterations"""
    from adaptive_sph_amd.workloads import dam_break_params
    return dam_break_params(hybrid_dfsph_max_avg_density_error=0.0, hybrid_dfsph_max_avg_divergence_error=0.0, iisph_max_avg_density_error=0.0, **kw)


MERGE_STEPS, MERGE_MAX_DT = 6, 2e-4
