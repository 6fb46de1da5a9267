"""The neighbour build -- cell keys, stable radix sort, reorder, cell-range table, and the two forms of the build queued ahead -- against
the CPU oracle at the shapes the workloads never produce (tests/neighbour_scenes.py builds them; tests/test_neighbour_build_scenes.py
proves on the CPU what each one exercises and that the checks below bite):

  a. every digit plan of radix_sort_pairs at both ends of its bit range (4 .. 25-bit cell keys), lattice-ordered and shuffled uploads;
  b. stability of the sort: a shuffled dense block under the EXACT policy is the oracle bit for bit in the device's order;
  c. tile and trip edges: n = 63 .. 2049, 1025 x 1025 (514 tiles, a one-key last tile) and 1449 x 1449 (1026 tiles: a second row-scan trip);
  d. the cell table: gaps of 63 / 64 / 65 cells around the inline threshold, a work list that overflows, stale entries of a larger scene;
  e. the grid limits: 65 532 cells along either axis, the refusal beyond 65 535 and what it leaves behind;
  f. the sorting grid of multi-resolution strips: the fine grid, twice its cell, the coarse grid as the fallback;
  g. the merge next to its admission limit and the radix form of the queued-ahead build just past it.

The common check after every step is test_gpu_parity.test_first_step_single_sweeps': dt, time and the sph_grid tuple equal; h2, cell_index,
neighbor_count, lambda_sum, lambda_grad_sum bit-exact; cell_index equal to the cells of the positions; neighbour SETS equal; density,
constant_field, aii within REL_TOL_SWEEP = 2e-5 (the project's bar); iteration counts forced (3, or 0 where the reference starts no
solve).  On the first step after an upload of a one-size scene the ORDER of every exported list is checked too: ascending slot of the
stable sort by cell.  No bar here is new."""
import numpy as np
import pytest

from adaptive_sph_amd import ffi
from tests import neighbour_scenes as ns
from tests import test_gpu_parity as parity
from tests.oracle_harness import cells_of_positions

pytestmark = pytest.mark.gpu

PARAMS = ns.forced_params(max_iters=3)
SPH_ERR_UNSUPPORTED, SPH_ERR_POISONED = 30, 31


def make_pair(product_lib, oracle_lib, scene, capacity=None, policy=None):
    n = capacity or len(scene["mass"])
    g, o = ffi.Context(product_lib, n, scene["planes"]), ffi.Context(oracle_lib, n, scene["planes"])
    if policy:
        g.set_math_policy(policy)
    g.profile_enable(1)
    upload(g, o, scene)
    return g, o


def upload(g, o, scene):
    g.upload(scene["mass"], scene["pos"], scene["vel"])
    o.upload(scene["mass"], scene["pos"], scene["vel"])


def grid_tuple(c):
    g = c.grid()
    return (g.cell_size, g.cells_min_x, g.cells_min_y, g.size_x, g.size_y)


def step_and_check(g, o, p, where, first=False, one_size=True, div_iters=None):
    """one step on both sides and the common check; `first`: the first step after an upload (the order check applies).  The iteration
    counts are FORCED (tolerances 0): a solve runs max_iters = 3 iterations or, where the reference finds nothing to solve -- clumps and
    blocks in free fall away from every wall have no divergence to remove -- none, on both sides alike; `div_iters`: the count a scene
    that stands on the floor must show."""
    x_before = o.download("position")
    sg, so = g.step(p), o.step(p)
    assert sg.dt == so.dt and sg.time == so.time, where
    assert grid_tuple(g) == grid_tuple(o), where
    for f in parity.BITEXACT:
        assert np.array_equal(g.download(f), o.download(f)), (where, f)
    ci = o.download("cell_index")
    assert np.array_equal(ci.astype(np.int64), cells_of_positions(x_before, o.grid())), where
    go, gi = g.download_neighbors()
    oo, oi = o.download_neighbors()
    assert np.array_equal(go, oo), where
    assert np.array_equal(ns.csr_keys(go, gi), ns.csr_keys(oo, oi)), where
    if first and one_size:
        assert ns.slot_order_violations(go, gi, ci) == 0, where
    errs = {f: parity.rel_err(g.download(f), o.download(f)) for f in parity.SWEEP_FIELDS}
    print(where, "n", len(ci), "grid", grid_tuple(o)[3:], {f: f"{e:.2e}" for f, e in errs.items()})
    for f, e in errs.items():
        assert e < parity.REL_TOL_SWEEP, (where, f, e)
    iters = (int(sg.div_solver.iters), int(sg.density_solver.iters))
    assert iters == (int(so.div_solver.iters), int(so.density_solver.iters)) and set(iters) <= {0, 3}, (where, iters)
    assert div_iters is None or iters[0] == div_iters, (where, iters)
    return sg, so


def launches(g, name):
    return g.profile_get().get(name, (0, 0.0))[0]


# ------------------------------------------------------------------------------------------------
# a. digit plans
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["lattice", "shuffled"])
@pytest.mark.parametrize("name", list(ns.PLAN_GRIDS))
def test_every_digit_plan_at_both_ends_of_its_bit_range(product_lib, oracle_lib, name, order):
    """Two steps: the first sorts by the reported grid (its digit plan: PLAN_GRIDS), queues the second's build ahead on that grid + 2 cells
    on every side -- a merge where the predicted grid holds at most n + 4096 cells, else the radix sort with clamped keys under the plan
    of THAT grid -- and the second step adopts it.  The launch counts say which plan ran: sort_scatter = passes."""
    scene = ns.plan_scene(name)
    if order == "shuffled":
        scene = ns.shuffled(scene)
    sx, sy = ns.PLAN_GRIDS[name]
    n = len(scene["mass"])
    first_passes = ns.digit_plan(sx * sy)[0]
    ahead_cells = (sx + 2 * ns.AHEAD_MARGIN) * (sy + 2 * ns.AHEAD_MARGIN)
    merged = ahead_cells <= n + ns.MERGE_SLACK
    ahead_passes = 0 if merged else ns.digit_plan(ahead_cells)[0]
    g, o = make_pair(product_lib, oracle_lib, scene)
    p = PARAMS.to_ffi()
    step_and_check(g, o, p, f"{name} {order} step 0:", first=True)
    assert grid_tuple(o)[3:] == (sx, sy)
    prof = g.profile_get()
    print(name, order, "after step 0", {k: prof[k][0] for k in ("sort_scatter", "inc_reorder", "cell_start", "reorder") if k in prof})
    assert launches(g, "sort_scatter") == first_passes + ahead_passes
    assert launches(g, "inc_reorder") == (1 if merged else 0) and launches(g, "cell_start") == (1 if merged else 2)
    step_and_check(g, o, p, f"{name} {order} step 1:")
    prof = g.profile_get()
    print(name, order, "after step 1", {k: prof[k][0] for k in ("sort_scatter", "inc_reorder", "cell_start", "reorder") if k in prof})
    # adopted: the second step sorted nothing at its start, and queued the third's build the same way
    assert launches(g, "sort_scatter") == first_passes + 2 * ahead_passes
    assert launches(g, "inc_reorder") == (2 if merged else 0) and launches(g, "cell_start") == (1 if merged else 3)
    g.close()
    o.close()


# ------------------------------------------------------------------------------------------------
# b. stability
# ------------------------------------------------------------------------------------------------
def test_shuffled_upload_sums_in_the_stable_order(product_lib, oracle_lib):
    """A dense block (4-5 particles per cell) uploaded SHUFFLED, EXACT policy: the device sorts it itself, and its neighbour sums run in
    ascending slot.  The oracle, given the same particles in the stable sort of the shuffled order by cell (test_gpu_bitexact.device_order),
    sums in ascending index = the same order if and only if the device's sort is stable: density, constant_field and aii bit for bit.  Two
    particles of one cell that changed places change the f32 sum order of every list that holds both."""
    from tests.test_gpu_bitexact import device_order, h_from_mass
    scene = ns.shuffled(ns.dense_block(96, 86), seed=7)
    n = len(scene["mass"])
    assert n == 8256
    order = device_order(scene["pos"], h_from_mass(scene["mass"]))
    assert (order != np.arange(n)).sum() > n // 2       # (the device's order is far from the upload order)
    g = ffi.Context(product_lib, n, scene["planes"])
    o = ffi.Context(oracle_lib, n, scene["planes"])
    g.set_math_policy("exact")
    g.upload(scene["mass"], scene["pos"], scene["vel"])
    o.upload(scene["mass"][order], scene["pos"][order], scene["vel"][order])
    p = PARAMS.to_ffi()
    sg, so = g.step(p), o.step(p)
    assert sg.dt == so.dt
    ci = g.download("cell_index")
    assert np.array_equal(ci[order], o.download("cell_index")) and (np.diff(ci[order].astype(np.int64)) >= 0).all()
    go, gi = g.download_neighbors()
    assert ns.slot_order_violations(go, gi, ci) == 0
    for f in ["neighbor_count", "density", "constant_field", "aii", "pressure", "position", "velocity"]:
        a, b = g.download(f)[order], o.download(f)
        assert np.array_equal(a, b), (f, int((a != b).reshape(n, -1).any(axis=1).sum()))
    g.close()
    o.close()


# ------------------------------------------------------------------------------------------------
# c. tile and trip edges
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(ns.EDGE_COUNTS))
def test_tile_edges(product_lib, oracle_lib, n):
    scene = ns.shuffled(ns.edge_scene(n), seed=n)
    g, o = make_pair(product_lib, oracle_lib, scene)
    p = PARAMS.to_ffi()
    step_and_check(g, o, p, f"n = {n} step 0:", first=True, div_iters=3)
    step_and_check(g, o, p, f"n = {n} step 1:", div_iters=3)
    g.close()
    o.close()


@pytest.mark.parametrize("side", [1025, 1449])
def test_large_lattice_shuffled(product_lib, oracle_lib, side):
    """1025 x 1025 = 1 050 625 particles: 514 tiles, the last one holds one key, and the row scan's last thread ends in mid-vector;
    1449 x 1449 = 2 099 601: 1026 tiles, a second row-scan trip of two tiles.  One step, uploaded shuffled (the time is the oracle's)."""
    from tests.oracle_harness import same_sets
    scene = ns.shuffled(ns.big_lattice(side), seed=side)
    g, o = make_pair(product_lib, oracle_lib, scene)
    p = PARAMS.to_ffi()
    sg, so = g.step(p), o.step(p)
    assert sg.dt == so.dt and grid_tuple(g) == grid_tuple(o)
    for f in parity.BITEXACT:
        assert np.array_equal(g.download(f), o.download(f)), f
    ci = o.download("cell_index")
    assert np.array_equal(ci.astype(np.int64), cells_of_positions(scene["pos"], o.grid()))
    same_sets(g, o)
    go, gi = g.download_neighbors()
    assert ns.slot_order_violations(go, gi, ci) == 0
    del go, gi
    for f in parity.SWEEP_FIELDS:
        e = parity.rel_err(g.download(f), o.download(f))
        print(side, f, f"{e:.2e}")
        assert e < parity.REL_TOL_SWEEP, f
    assert sg.div_solver.iters == so.div_solver.iters == 3
    g.close()
    o.close()


# ------------------------------------------------------------------------------------------------
# d. the cell table
# ------------------------------------------------------------------------------------------------
def test_cell_table_threshold_overflow_and_stale_entries(product_lib, oracle_lib):
    """ONE context: a dense block (a table of real, non-zero entries), the sparse scene whose gaps between occupied keys are 63 (inline), 64
    and 65 cells (work list), the scene with more long gaps than the work list holds (the rest falls back to the inline loop), and the
    sparse scene again -- its table now lies inside the larger scene's, every entry of it stale.  Two steps each."""
    big = ns.table_overflow_scene()
    cap = len(big["mass"])
    stages = [("dense", ns.dense_block(64, 64)), ("threshold", ns.shuffled(ns.table_threshold_scene(), seed=3)), ("overflow", big),
              ("threshold after overflow", ns.table_threshold_scene())]
    # (one box for all four: the widest scene's, so that no particle of any stage stands near or beyond a wall)
    for _, scene in stages:
        scene["planes"] = big["planes"]
    g, o = make_pair(product_lib, oracle_lib, stages[0][1], capacity=cap)
    p = PARAMS.to_ffi()
    for k, (what, scene) in enumerate(stages):
        if k:
            upload(g, o, scene)
        before = launches(g, "cell_start")
        step_and_check(g, o, p, f"{what} step 0:", first=True)
        step_and_check(g, o, p, f"{what} step 1:")
        assert launches(g, "cell_start") > before        # (k_cell_start / k_cell_fill ran for this scene)
    g.close()
    o.close()


# ------------------------------------------------------------------------------------------------
# e. grid limits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transpose", [False, True])
def test_grid_just_below_the_limit_and_the_refusal_beyond_it(product_lib, oracle_lib, transpose):
    """65 532 cells along one axis: cx | cy << 16 carries a full 16-bit coordinate (the grid queued ahead would not fit: every step builds
    at its start).  65 540: SPH_ERR_UNSUPPORTED naming the cell grid, taken before anything of the build is launched -- the context is as
    it was (include/sph_ffi.h): the same answer again, not SPH_ERR_POISONED, the uploaded particles untouched, and the context goes on
    with another scene."""
    scene = ns.shuffled(ns.limit_scene(ns.LIMIT_FITS, transpose), seed=11)
    g, o = make_pair(product_lib, oracle_lib, scene)
    p = PARAMS.to_ffi()
    step_and_check(g, o, p, "below the limit step 0:", first=True)
    assert max(grid_tuple(o)[3:]) == ns.LIMIT_FITS
    step_and_check(g, o, p, "below the limit step 1:")
    assert launches(g, "sort_scatter") == 2 * ns.digit_plan(8 * ns.LIMIT_FITS)[0] and launches(g, "inc_reorder") == 0
    too_wide = ns.limit_scene(ns.LIMIT_REFUSED, transpose)
    g.upload(too_wide["mass"], too_wide["pos"], too_wide["vel"])
    for attempt in range(2):
        with pytest.raises(ffi.SphError) as err:
            g.step(p)
        print("refusal", attempt, err.value)
        assert err.value.status == SPH_ERR_UNSUPPORTED and "cell grid" in str(err.value) and "too large" in str(err.value), attempt
    for f, want in (("mass", too_wide["mass"]), ("position", too_wide["pos"]), ("velocity", too_wide["vel"])):
        assert np.array_equal(g.download(f), want), f
    small = ns.plan_scene("bits09")
    upload(g, o, small)
    step_and_check(g, o, p, "after the refusal step 0:", first=True)
    step_and_check(g, o, p, "after the refusal step 1:")
    g.close()
    o.close()


# ------------------------------------------------------------------------------------------------
# f. multi-resolution sorting grid
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ns.MULTIRES_SCENES))
def test_multiresolution_strips(product_lib, oracle_lib, name):
    extent, ratio, doublings, tile = ns.MULTIRES_SCENES[name]
    scene = ns.two_size_strip(extent, ratio)
    n = len(scene["mass"])
    g, o = make_pair(product_lib, oracle_lib, scene)
    p = PARAMS.to_ffi()
    for s in range(3):
        step_and_check(g, o, p, f"{name} step {s}:", one_size=False)
        forms = g.profile_list_forms()
        print(name, s, forms)
        assert forms["n_lists"] == n == forms["n_mask"] + forms["n_index"] + forms["n_walk"], forms
    assert launches(g, "tile_hmax") >= 3       # sorted by a grid of its own, tiles bound the neighbours' h
    g.close()
    o.close()


# ------------------------------------------------------------------------------------------------
# g. the merge at its admission limit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("admitted", [True, False])
def test_merge_next_to_its_admission_limit(product_lib, oracle_lib, admitted):
    """Two blocks moving towards each other, the predicted grid a column or two below / above n + 4096 cells (CPU module): below, every
    build after the first is the merge; above, every one is the radix sort queued ahead with clamped keys on the predicted grid, adopted by
    the next step.  The oracle is the reference at every step."""
    scene = ns.two_blocks(ns.merge_gap_for(32, admitted))
    g, o = make_pair(product_lib, oracle_lib, scene)
    p = ns.forced_params(max_iters=3, max_dt=ns.MERGE_MAX_DT).to_ffi()
    scatter = []
    for s in range(ns.MERGE_STEPS):
        step_and_check(g, o, p, f"admitted {admitted} step {s}:", first=s == 0)
        scatter.append(launches(g, "sort_scatter"))
        print("admitted", admitted, s, "sort_scatter", scatter[-1], "inc_reorder", launches(g, "inc_reorder"), "cell_start", launches(g, "cell_start"))
    ok, rep = parity.displacement_bars(g.download("position"), o.download("position"), scene["pos"])
    assert ok, rep
    passes = 2        # 13-bit keys either way
    if admitted:
        assert launches(g, "inc_reorder") == ns.MERGE_STEPS and scatter == [passes] * ns.MERGE_STEPS
    else:
        assert launches(g, "inc_reorder") == 0 and scatter == [passes * (s + 2) for s in range(ns.MERGE_STEPS)]
    g.close()
    o.close()
