"""TEST-ONLY helpers around the CPU oracle (oracle/).  Nothing in the product package imports this."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from adaptive_sph_amd import ffi

REPO = Path(__file__).resolve().parent.parent
ORACLE_DIR = REPO / "oracle"
ORACLE_LIB = ORACLE_DIR / "liboracle.so"

_ORACLE = None


def build_oracle():
    r = subprocess.run(["make", "-C", str(ORACLE_DIR)], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("oracle build failed:\n" + r.stdout + r.stderr)
    return ORACLE_LIB


def load_oracle() -> ffi.SphLibrary:
    global _ORACLE
    if _ORACLE is None:
        build_oracle()
        lib = ffi.SphLibrary(ORACLE_LIB, "oracle_")
        L = lib.lib
        L.oracle_cubic_kernel_2d.restype = C.c_float
        L.oracle_cubic_kernel_2d.argtypes = [C.c_float, C.c_float]
        L.oracle_cubic_kernel_2d_deriv.restype = None
        L.oracle_cubic_kernel_2d_deriv.argtypes = [C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        for nm in ("oracle_sphere_volume_to_radius", "oracle_radius_to_sphere_volume"):
            getattr(L, nm).restype = C.c_float
            getattr(L, nm).argtypes = [C.c_float]
        L.oracle_h_from_mass.restype = C.c_float
        L.oracle_h_from_mass.argtypes = [C.c_float, C.c_float]
        for nm in ("oracle_lambda2", "oracle_dlambda2"):
            getattr(L, nm).restype = C.c_double
            getattr(L, nm).argtypes = [C.c_double]
        L.oracle_lambda_luts.restype = None
        L.oracle_lambda_luts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.oracle_lut_get.restype = C.c_float
        L.oracle_lut_get.argtypes = [C.c_void_p, C.c_int, C.c_float]
        L.oracle_add_fluid_block.restype = C.c_uint64
        L.oracle_add_fluid_block.argtypes = [C.c_float] * 8 + [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.oracle_boundary_box.restype = None
        L.oracle_boundary_box.argtypes = [C.c_float, C.c_float, C.POINTER(ffi.SphPlane)]
        L.oracle_build_neighbors.restype = C.c_int
        L.oracle_build_neighbors.argtypes = [C.c_void_p, C.c_float]
        L.oracle_check_neighborhood.restype = C.c_int
        L.oracle_check_neighborhood.argtypes = [C.c_void_p]
        L.oracle_num_threads.restype = C.c_int
        L.oracle_set_num_threads.argtypes = [C.c_int]
        _ORACLE = lib
    return _ORACLE


def oracle_kernel_deriv(lib, dx, dy, h):
    gx, gy = C.c_float(), C.c_float()
    lib.lib.oracle_cubic_kernel_2d_deriv(dx, dy, h, C.byref(gx), C.byref(gy))
    return gx.value, gy.value


def oracle_scene_block(lib, block):
    """add_fluid_block through the oracle's own C restatement."""
    args = [block.pos[0], block.pos[1], block.size[0], block.size[1], block.spacing, block.volume_fill_ratio,
            block.velocity[0], block.velocity[1]]
    n = int(lib.lib.oracle_add_fluid_block(*args, 0, None, None, None))
    pos = np.empty((n, 2), np.float32)
    mass = np.empty(n, np.float32)
    vel = np.empty((n, 2), np.float32)
    lib.lib.oracle_add_fluid_block(*args, n, pos.ctypes.data, mass.ctypes.data, vel.ctypes.data)
    return pos, mass, vel


def oracle_box(lib, width, height):
    arr = (ffi.SphPlane * 4)()
    lib.lib.oracle_boundary_box(width, height, arr)
    return [(p.dir_x, p.dir_y, p.delta) for p in arr]


def csr_sets(offsets, indices):
    """list of sorted index arrays per particle"""
    return [np.sort(indices[offsets[i]:offsets[i + 1]]) for i in range(len(offsets) - 1)]


def uniform_params(**kw):
    """default-config.yaml with the uniform dam-break overrides of SURVEY.md section 8d config 2
    (media/motivation-video.yaml:42-57)."""
    from adaptive_sph_amd.workloads import dam_break_params
    return dam_break_params(**kw)


def ring_scene(n_ring=20, h=0.05, radius_in_h=1.2, centre=(0.0, 0.0), jitter=0.0, seed=0):
    """A particle in the middle of a ring of `n_ring` others at ~1.2 h: n_ring + 1 entries on its list (> 19) and every fringe
    value 2 |x_ij| - 2 h_j in [0, h) -- the one geometry in which constrain_neighborhood_count (simulation.rs:2145-2177)
    passes its own two assertions.  The ring particles see at most ~17 neighbours and keep their h.  `jitter` spreads the
    ring radii (distinct fringe values)."""
    rng = np.random.default_rng(seed)
    ang = np.arange(n_ring, dtype=np.float64) * (2 * np.pi / n_ring)
    rad = radius_in_h * h * (1.0 + jitter * rng.uniform(-1.0, 1.0, n_ring))
    pos = np.zeros((n_ring + 1, 2), np.float32)
    pos[:, 0] = centre[0]
    pos[:, 1] = centre[1]
    pos[1:, 0] += (rad * np.cos(ang)).astype(np.float32)
    pos[1:, 1] += (rad * np.sin(ang)).astype(np.float32)
    m = np.float32(np.pi * (h / 1.9) ** 2)            # h = 1.9 sqrt(m / pi) at rest_density 1
    mass = np.full(n_ring + 1, m, np.float32)
    vel = np.zeros((n_ring + 1, 2), np.float32)
    return pos, mass, vel


def rings_and_block_scene():
    """Three jittered rings (21, 23, 25 list entries in the middle: ranks 2, 4, 6 of the descending fringe order) beside a
    rest-lattice block in which nobody exceeds 19 neighbours."""
    from adaptive_sph_amd import scene as sc
    parts = [ring_scene(20, 0.05, 1.2, (-1.0, 0.5), 0.08, 1), ring_scene(22, 0.04, 1.2, (0.0, 0.6), 0.08, 2),
             ring_scene(24, 0.06, 1.2, (1.0, 0.4), 0.08, 3)]
    scn = sc.dam_break_small(24, 24, 1 / 24)
    parts.append(sc.init_particles(scn))
    pos = np.concatenate([p[0] for p in parts]).astype(np.float32)
    mass = np.concatenate([p[1] for p in parts]).astype(np.float32)
    vel = np.concatenate([p[2] for p in parts]).astype(np.float32)
    return scn, pos, mass, vel


def quadtree_scene(seed):
    rng = np.random.default_rng(seed)
    levels = int(rng.integers(1, 6))                 # size ratio up to 32:1
    s_max = float(rng.choice([0.08, 0.1, 0.16]))
    kind = int(rng.integers(0, 4))
    w, hgt = float(rng.uniform(0.8, 2.4)), float(rng.uniform(0.5, 1.4))
    x0, y0 = -1.95 + float(rng.uniform(0, 0.3)), -0.95 + float(rng.uniform(0, 0.2))
    cx, cy = x0 + w * rng.uniform(0.2, 0.8), y0 + hgt * rng.uniform(0.2, 0.8)
    ang = rng.uniform(0, np.pi)

    def size_at(x, y):          # wanted particle spacing
        if kind == 0:           # fine disc in a coarse bath
            d = np.hypot(x - cx, y - cy)
            t = np.clip(d / (0.35 * min(w, hgt)), 0, 1)
        elif kind == 1:         # sharp slanted interface
            t = 1.0 if (x - cx) * np.cos(ang) + (y - cy) * np.sin(ang) > 0 else 0.0
        elif kind == 2:         # smooth gradient
            t = np.clip((x - x0) / w, 0, 1)
        else:                   # fine layer at the top ("free surface")
            t = np.clip((y0 + hgt - y) / (0.5 * hgt), 0, 1)
        return s_max * 2.0 ** (-levels * (1.0 - t))

    pts, sizes = [], []

    def rec(x, y, s, depth):
        if depth < levels and size_at(x + s / 2, y + s / 2) < s / 1.41:
            for dx in (0, 1):
                for dy in (0, 1):
                    rec(x + dx * s / 2, y + dy * s / 2, s / 2, depth + 1)
        else:
            j = rng.uniform(-0.15, 0.15, 2) * s
            pts.append((x + s / 2 + j[0], y + s / 2 + j[1]))
            sizes.append(s)

    nx, ny = max(int(w / s_max), 1), max(int(hgt / s_max), 1)
    for ix in range(nx):
        for iy in range(ny):
            rec(x0 + ix * s_max, y0 + iy * s_max, s_max, 0)
    pos = np.array(pts, np.float32)
    sizes = np.array(sizes, np.float32)
    mass = (np.float32(0.93) * sizes * sizes).astype(np.float32)
    vel = (rng.normal(0, 0.05, pos.shape)).astype(np.float32)
    return pos, mass, vel, dict(levels=levels, kind=kind, s_max=s_max)


def displacement_bars(x_gpu, x_oracle, x0, rel=1e-3):
    """Positions compared through the DISPLACEMENT from the uploaded positions x0 -- relative to max|x| (~2) a bar of 1e-4 is
    0.2 mm absolute, more than a particle at rest-lattice spacing 1/1024 moves in the first steps, so that bar alone cannot fail.
    Two figures, both against `rel` x the oracle's own displacement plus ONE ulp of the largest coordinate (positions are f32: two
    correct integrations may round a coordinate to neighbouring floats, and that quantum is 2e-3 of a 6e-5 displacement):
      * max over the particles of |dx_gpu - dx_oracle|  vs  rel * max|dx_oracle|  (the fastest particles)
      * median of the same                              vs  rel * median|dx_oracle|  (the bulk, which the ejected corners do not hide)
    Returns (ok, report); `report` carries the numbers for the assertion message.  A kernel that never moved a particle has
    error == displacement and fails both by three orders of magnitude."""
    xg, xo, x0 = (np.asarray(a, np.float64) for a in (x_gpu, x_oracle, x0))
    dg, do = xg - x0, xo - x0
    err = np.abs(dg - do).max(axis=1)
    mag = np.abs(do).max(axis=1)
    ulp = float(np.spacing(np.float32(np.abs(xo).max())))
    rep = {"max_err": float(err.max()), "max_disp": float(mag.max()), "median_err": float(np.median(err)), "median_disp": float(np.median(mag)), "ulp": ulp}
    meaningful = rep["max_disp"] > 50 * ulp and rep["median_disp"] > 10 * ulp      # the scene moved by more than rounding
    ok = meaningful and rep["max_err"] <= rel * rep["max_disp"] + ulp and rep["median_err"] <= rel * rep["median_disp"] + ulp
    return ok, rep


def same_sets(g, o):
    """Equal CSR offsets, per particle equal sums and sums of squares of the neighbour indices (a cheap first look), then the SETS
    entry by entry: the order inside a list is unspecified (cell-sorted on the device, ascending in the oracle)."""
    go, gi = g.download_neighbors()
    oo, oi = o.download_neighbors()
    assert np.array_equal(go, oo)
    starts = go[:-1].astype(np.int64)
    assert (np.diff(go.astype(np.int64)) > 0).all()          # every particle is on its own list
    for power in (1, 2):
        a = np.add.reduceat(gi.astype(np.uint64) ** power, starts)
        b = np.add.reduceat(oi.astype(np.uint64) ** power, starts)
        assert np.array_equal(a, b), power
    # ... and the sets themselves: (row, index) packed into one 64-bit key per entry, the device's entries sorted (the oracle's lists
    # are ascending already), compared whole -- 13 M entries at configs[1], 110 M at configs[3]
    rows = np.repeat(np.arange(len(go) - 1, dtype=np.uint64), np.diff(go.astype(np.int64))) << np.uint64(32)
    key_o = rows | oi.astype(np.uint64)
    assert (np.diff(key_o.astype(np.int64)) > 0).all()
    key_g = rows | gi.astype(np.uint64)
    key_g.sort()
    assert np.array_equal(key_g, key_o)


# ------------------------------------------------------------------------------------------------
# The neighbour-list FORM of every particle, predicted on the host (tests/test_gpu_list_forms.py, tests/test_list_form_predictor.py).
# The density (BUILD) sweep of adaptive_sph_amd/csrc/sph_sweeps.hip decides per particle and step how the later sweeps read its
# neighbours; the thresholds below restate that decision in numpy for scenes of ONE particle size (3 x 3 stencil everywhere).
# ------------------------------------------------------------------------------------------------
ROW_CAP = 32          # candidates per row of three cells a mask word can address (sweep_particle: ok_list)
INDEX_CAP = 128       # NLX_CAP: entries of an explicit index list
OFFSET_SLOTS = 24     # NLOFF_SLOTS: 16-bit offsets per particle, the particle itself not counted
OFFSET_MIN, OFFSET_MAX = -32768, 32767
MAX_NEIGHBOR_COUNT = 20000   # SPH_ERR_TOO_MANY_NEIGHBORS above it (neighborhood_search.rs:3)
FORM_MASK, FORM_INDEX, FORM_WALK = 0, 1, 2


def squeeze_about_first(pos, factor_x, factor_y=None):
    """the lattice squeezed about its first particle, masses (so h and the grid) unchanged"""
    f = np.array([factor_x, factor_x if factor_y is None else factor_y], np.float32)
    return (pos[0] + (pos - pos[0]) * f).astype(np.float32)


def half_squeezed_scene(nx=64, ny=40, spacing=1 / 48, fx=0.5, fy=0.6):
    """dam_break_small(nx, ny): the right half squeezed (fx along x about the middle column, fy along y about the bottom row), the left
    half at rest spacing -- mask lanes and walk lanes in the same scene and, along the seam, in the same waves"""
    from adaptive_sph_amd import scene as sc
    scn = sc.dam_break_small(nx, ny, spacing)
    pos, mass, vel = sc.init_particles(scn)
    x0, y0 = pos[:, 0].min(), pos[:, 1].min()
    mid = np.float32(x0 + (nx // 2) * spacing)
    right = pos[:, 0] > mid
    out = pos.copy()
    out[right, 0] = mid + (pos[right, 0] - mid) * np.float32(fx)
    out[right, 1] = y0 + (pos[right, 1] - y0) * np.float32(fy)
    return scn, out.astype(np.float32), mass, vel


def device_slots(cell_index):
    """slot of every host particle in the device's cell-sorted order on the FIRST step after an upload: stable sort by cell"""
    order = np.argsort(np.asarray(cell_index).astype(np.int64), kind="stable")
    slot = np.empty(len(order), np.int64)
    slot[order] = np.arange(len(order))
    return slot


def candidate_rows(grid, cell_index):
    """(n, 3) candidates in the three rows of three cells around every particle: cells max(cx - 1, 0) .. min(cx + 1, sx - 1) of the rows
    cy - 1, cy, cy + 1, a row outside the grid holding none (sweep_particle's clamps, through the same exclusive cell-start table)"""
    sx, sy = int(grid.size_x), int(grid.size_y)
    ci = np.asarray(cell_index).astype(np.int64)
    assert ci.min() >= 0 and ci.max() < sx * sy
    start = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=sx * sy))])
    cx, cy = ci % sx, ci // sx
    rows = np.zeros((len(ci), 3), np.int64)
    for dr in range(3):
        yy = cy + dr - 1
        ok = (yy >= 0) & (yy < sy)
        base = np.where(ok, yy, 0) * sx
        rows[:, dr] = np.where(ok, start[base + np.minimum(cx + 2, sx)] - start[base + np.maximum(cx - 1, 0)], 0)
    return rows


def cells_of_positions(pos, grid):
    """cell index from the position: floor(x / cell_size) in IEEE f32, x fastest (neighborhood_search.rs:253-255, :383-395)"""
    cs = np.float32(grid.cell_size)
    cx = np.floor(pos[:, 0].astype(np.float32) / cs).astype(np.int64) - int(grid.cells_min_x)
    cy = np.floor(pos[:, 1].astype(np.float32) / cs).astype(np.int64) - int(grid.cells_min_y)
    return cx + cy * int(grid.size_x)


def predict_list_forms(grid, cell_index, neighbor_count, lambda_sum, policy="fast", extended=False):
    """The form every particle of a ONE-SIZE scene takes, host order: (form array, counts dict as profile_list_forms() reports them).
       mask   every row <= 32 candidates (never for the level estimation's extended lists);
       index  else, where index lists are recorded (EXACT math, extended lists) and the list holds <= 128 entries, self included;
       walk   else.
    `neighbor_count`: the oracle's, self included (of the extended lists when `extended`)."""
    rows = candidate_rows(grid, cell_index)
    nc = np.asarray(neighbor_count).astype(np.int64)
    ok_list = (rows <= ROW_CAP).all(axis=1) & (not extended)
    records = policy == "exact" or extended
    form = np.where(ok_list, FORM_MASK, np.where(records & (nc <= INDEX_CAP), FORM_INDEX, FORM_WALK))
    counts = {"n_lists": len(nc), "n_mask": int((form == FORM_MASK).sum()), "n_index": int((form == FORM_INDEX).sum()),
              "n_walk": int((form == FORM_WALK).sum()), "n_wall": int((np.asarray(lambda_sum) != 0).sum())}
    return form, counts


def offset_ranges(cell_index, offsets, indices):
    """per particle (smallest, largest) slot difference j - i over its neighbours in the device's cell-sorted order (0 with no neighbour
    but itself) -- what emit_offset_list stores in 16 bits"""
    slot = device_slots(cell_index)
    off = np.asarray(offsets).astype(np.int64)
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    d = slot[np.asarray(indices).astype(np.int64)] - slot[rows]
    lo = np.minimum.reduceat(d, off[:-1])
    hi = np.maximum.reduceat(d, off[:-1])
    return lo, hi


def predict_offset_lists(form, cell_index, offsets, indices):
    """which particles get a 16-bit offset list under the FAST policy: a mask word, <= 24 neighbours besides the particle itself, every
    slot difference within int16.  Returns (has_list, lo, hi)."""
    lo, hi = offset_ranges(cell_index, offsets, indices)
    others = np.diff(np.asarray(offsets).astype(np.int64)) - 1
    return (form == FORM_MASK) & (others <= OFFSET_SLOTS) & (lo >= OFFSET_MIN) & (hi <= OFFSET_MAX), lo, hi


def mixed_waves(form, cell_index, a=FORM_MASK, b=FORM_WALK):
    """number of 64-slot waves of the cell-sorted order that hold both forms"""
    slot = device_slots(cell_index)
    wave = slot // 64
    nw = int(wave.max()) + 1
    return int(((np.bincount(wave[form == a], minlength=nw) > 0) & (np.bincount(wave[form == b], minlength=nw) > 0)).sum())


def squeezed_scene(factor, jitter=0.0, seed=0, nx=48, ny=40, spacing=1 / 48):
    """dam_break_small(nx, ny) squeezed about its first particle (the block's lower left corner, beside the box's), optionally jittered
    by +-`jitter` lattice spacings with a fixed seed"""
    from adaptive_sph_amd import scene as sc
    scn = sc.dam_break_small(nx, ny, spacing)
    pos, mass, vel = sc.init_particles(scn)
    pos = squeeze_about_first(pos, factor)
    if jitter:
        rng = np.random.default_rng(seed)
        pos = (pos + rng.uniform(-jitter, jitter, pos.shape).astype(np.float32) * np.float32(factor * spacing)).astype(np.float32)
    return scn, pos, mass, vel


def corners_scene(factor=0.45):
    """squeezed_scene(factor) in the box's lower left corner and its point mirror in the upper right one: crowded particles with wall terms
    in the first AND the last occupied column and row of the grid"""
    scn, pos, mass, vel = squeezed_scene(factor)
    return scn, np.concatenate([pos, -pos]).astype(np.float32), np.concatenate([mass, mass]), np.concatenate([vel, vel])


LIST_FORM_SCENES = {
    "squeeze_0.60": lambda: squeezed_scene(0.60),
    "squeeze_0.55": lambda: squeezed_scene(0.55),
    "squeeze_0.45": lambda: squeezed_scene(0.45),
    "half_squeezed": half_squeezed_scene,
    "rows_32_33": lambda: squeezed_scene(0.57, 0.1, 0),      # rows of exactly 32 and 33 candidates, lists of exactly 24 and 25 others
    "index_128_129": lambda: squeezed_scene(0.32, 0.2, 0),   # lists of exactly 128 and 129 entries
    "corners": corners_scene,
}


def strip_scene(nx=15800, ny=6, spacing=1 / 64):
    """a strip of nx x ny particles in a box wide enough to hold it: three cell rows of nx, 3 nx and 2 nx particles, so the slot
    difference to the adjacent row runs linearly along the strip and crosses -32768 / +32767 inside it"""
    from adaptive_sph_amd import scene as sc
    width = 2.0 * np.ceil(nx * spacing / 2.0 + 2.0)
    off, eps = spacing * 1.024, spacing * 0.5
    return sc.SceneConfig(sc.SceneBoundary("box", float(width), 2.0),
                          [sc.SceneFluidBlock([-width / 2 + off, -1.0 + off], [nx * spacing + eps, ny * spacing + eps], spacing, 0.93, [0.0, 0.0])])


def cluster_scene(n_others, h=0.05, radius_in_h=1.95, centre=(0.0, 0.0)):
    """one particle in the middle of `n_others` equal ones spread evenly over a circle of radius 1.95 h < 2 h: its list holds all of them
    and itself, theirs the arc within reach (about a third of the circle)"""
    ang = np.arange(n_others, dtype=np.float64) * (2 * np.pi / n_others)
    pos = np.zeros((n_others + 1, 2), np.float64) + np.asarray(centre, np.float64)
    pos[1:, 0] += radius_in_h * h * np.cos(ang)
    pos[1:, 1] += radius_in_h * h * np.sin(ang)
    mass = np.full(n_others + 1, np.float32(np.pi * (h / 1.9) ** 2), np.float32)
    return pos.astype(np.float32), mass, np.zeros((n_others + 1, 2), np.float32)


def list_form_facts(ctx, pos, policy="fast"):
    """What a scene exercises, from the ORACLE's first step alone (`ctx`: an oracle context after one step of `pos` uploaded in host
    order): the predicted forms and the counts the threshold tests rely on."""
    g, ci = ctx.grid(), ctx.download("cell_index")
    nc, lam = ctx.download("neighbor_count").astype(np.int64), ctx.download("lambda_sum")
    assert np.array_equal(ci.astype(np.int64), cells_of_positions(pos, g))
    off, idx = ctx.download_neighbors()
    assert np.array_equal(np.diff(off.astype(np.int64)), nc)
    form, counts = predict_list_forms(g, ci, nc, lam, policy)
    rows = candidate_rows(g, ci).max(axis=1)
    has_list, lo, hi = predict_offset_lists(form, ci, off, idx)
    mask, walk = form == FORM_MASK, form == FORM_WALK
    sx = int(g.size_x)
    cx, cy = ci.astype(np.int64) % sx, ci.astype(np.int64) // sx
    wallwalk = walk & (lam != 0)
    facts = dict(counts=counts, form=form, has_list=has_list, lo=lo, hi=hi, n=len(nc), neighbor_count=nc,
                 rows_32=int((rows == ROW_CAP).sum()), rows_33=int((rows == ROW_CAP + 1).sum()),
                 others_24=int((mask & (nc - 1 == OFFSET_SLOTS)).sum()), others_25=int((mask & (nc - 1 == OFFSET_SLOTS + 1)).sum()),
                 list_128=int((~mask & (nc == INDEX_CAP)).sum()), list_129=int((~mask & (nc == INDEX_CAP + 1)).sum()),
                 mask_walk_waves=mixed_waves(form, ci), index_walk_waves=mixed_waves(form, ci, FORM_INDEX, FORM_WALK),
                 # (the grid keeps one empty cell around the particles: columns 1 and sx - 2, rows 1 and sy - 2 are the outermost
                 #  occupied ones; their candidate ranges begin / end exactly where sweep_particle's clamps do)
                 wall_walk_edges=(int((wallwalk & (cx == cx.min())).sum()), int((wallwalk & (cx == cx.max())).sum()),
                                  int((wallwalk & (cy == cy.min())).sum()), int((wallwalk & (cy == cy.max())).sum())),
                 occupied=(int(cx.min()), int(cx.max()), int(cy.min()), int(cy.max())), grid=(sx, int(g.size_y)))
    return facts


def _share(facts, key, least_share=0.2, least=500):
    c = facts["counts"][key]
    return c >= least and c >= least_share * facts["n"]


# what every scene must exercise (policy -> predicate over list_form_facts): checked on the CPU (tests/test_list_form_predictor.py) and
# again beside the device's counts (tests/test_gpu_list_forms.py).  A targeted form holds >= 20 % of the particles and >= 500.
LIST_FORM_REQUIREMENTS = {
    "squeeze_0.60": {"fast": lambda f: _share(f, "n_walk") and _share(f, "n_mask"), "exact": lambda f: _share(f, "n_index")},
    "squeeze_0.55": {"fast": lambda f: _share(f, "n_walk"), "exact": lambda f: _share(f, "n_index")},
    "squeeze_0.45": {"fast": lambda f: _share(f, "n_walk") and min(f["wall_walk_edges"][0], f["wall_walk_edges"][2]) > 0, "exact": lambda f: _share(f, "n_index")},
    "half_squeezed": {"fast": lambda f: _share(f, "n_walk") and _share(f, "n_mask") and f["mask_walk_waves"] > 0,
                      "exact": lambda f: _share(f, "n_index") and _share(f, "n_mask")},
    "rows_32_33": {"fast": lambda f: _share(f, "n_walk") and min(f["rows_32"], f["rows_33"], f["others_24"], f["others_25"]) > 0,
                   "exact": lambda f: _share(f, "n_index") and min(f["rows_32"], f["rows_33"]) > 0},
    "index_128_129": {"fast": lambda f: _share(f, "n_walk"),
                      "exact": lambda f: _share(f, "n_index") and _share(f, "n_walk") and min(f["list_128"], f["list_129"]) > 0 and f["index_walk_waves"] > 0},
    "corners": {"fast": lambda f: _share(f, "n_walk") and min(f["wall_walk_edges"]) > 0 and f["occupied"] == (1, f["grid"][0] - 2, 1, f["grid"][1] - 2),
                "exact": lambda f: _share(f, "n_index")},
}


def assert_strip_crossings(facts, pos, grid, cell_index, nx=15800):
    """strip_scene: three cell rows of nx / 3 nx / 2 nx particles.  At the fraction t of the strip's length the rows below / above a
    particle begin about  t P_own + (1 - t) P_below  slots before it /  (1 - t) P_own + t P_above  slots behind it, so
      * bottom row (P = nx, above it 3 nx): the offsets to the row above pass +32767 at t = (32767 - nx) / (2 nx): offset lists left of
        it, mask words right of it;
      * top row (P = 2 nx, below it 3 nx): the offsets to the row below pass -32768 at t = (3 nx - 32768) / nx: mask words left of it,
        offset lists right of it.
    (The particle rows of one cell row reach different neighbours: the change-over takes a column or two.)
    Asserted: both kinds of lane exist, both limits are exceeded, and each crossing lies within 64 columns of that estimate."""
    has, lo, hi = facts["has_list"], facts["lo"], facts["hi"]
    cy = np.asarray(cell_index).astype(np.int64) // int(grid.size_x)
    rows = np.unique(cy)
    assert len(rows) == 3 and [int((cy == r).sum()) for r in rows] == [nx, 3 * nx, 2 * nx]
    assert has.sum() > 5000 and (~has).sum() > 5000
    assert (lo < OFFSET_MIN).sum() > 5000 and (hi > OFFSET_MAX).sum() > 5000 and lo.min() >= -3 * nx - 64 and hi.max() <= 3 * nx + 64
    # lanes sit exactly one slot beyond either limit: a range test that is off by one would give them a list
    assert (lo == OFFSET_MIN - 1).any() and (hi == OFFSET_MAX + 1).any()
    x = pos[:, 0].astype(np.float64)
    col = np.rint((x - x.min()) / ((x.max() - x.min()) / (nx - 1))).astype(np.int64)
    # (the lanes that have a neighbour in the adjacent cell row at all: a difference inside one's own row stays below ~100 slots)
    bottom, top = (cy == rows[0]) & (hi > 1000), (cy == rows[2]) & (lo < -1000)
    assert bottom.sum() >= nx and top.sum() >= nx
    # bottom row: nothing below it, the positive limit alone decides
    assert (has | (hi > OFFSET_MAX))[bottom].all() and col[bottom & has].max() <= col[bottom & ~has].min() + 2
    assert abs(col[bottom & has].max() - (OFFSET_MAX - nx) / 2.0) <= 64
    # top row: the negative limit alone
    assert (has | (lo < OFFSET_MIN))[top].all() and col[top & ~has].max() <= col[top & has].min() + 2
    assert abs(col[top & has].min() - (3 * nx + OFFSET_MIN)) <= 64
    return int(col[bottom & has].max()), int(col[top & has].min())
