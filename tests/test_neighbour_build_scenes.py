"""What the scenes of tests/test_gpu_neighbour_build.py exercise, proved on the CPU from the positions, the oracle's first step and numpy
alone (the role tests/test_list_form_predictor.py has for the list forms): grid dimensions and digit plan, tile and trip counts, the
gaps between occupied cell keys on either side of the inline / work-list threshold and beyond the work list's capacity, the grid
limits, the sorting grid of the multi-resolution strips, the admission of the merge.  The oracle itself is checked on them --
cell_index against the positions, neighbour sets against a brute force that knows no grid -- and the GPU module's order check and set
check are shown to bite on defects made in numpy: no broken kernel is ever run."""
import functools

import numpy as np
import pytest

from adaptive_sph_amd import ffi
from tests import neighbour_scenes as ns
from tests.oracle_harness import cells_of_positions, load_oracle

PARAMS = ns.forced_params(max_iters=3)


def oracle_steps(scene, steps=1, params=PARAMS):
    """per step: (positions before it, grid tuple, cell_index); and the lists of the LAST step"""
    o = ffi.Context(load_oracle(), len(scene["mass"]), scene["planes"])
    o.upload(scene["mass"], scene["pos"], scene["vel"])
    p = params.to_ffi()
    out = []
    for _ in range(steps):
        x = o.download("position")
        o.step(p)
        g = o.grid()
        ci = o.download("cell_index").astype(np.int64)
        assert np.array_equal(ci, cells_of_positions(x, g))       # the oracle's cells are the positions' cells
        out.append((x, (int(g.size_x), int(g.size_y)), ci))
    off, idx = o.download_neighbors()
    o.close()
    return out, (off, idx)


@functools.lru_cache(maxsize=None)
def first_step(builder, *args):
    scene = builder(*args)
    steps, lists = oracle_steps(scene)
    return scene, steps[0][1], steps[0][2], lists


def assert_sets_are_brute_force(scene, lists):
    assert np.array_equal(ns.csr_keys(*lists), ns.brute_force_keys(scene))


def test_the_constants_restated_here_are_the_products():
    c = ns.product_constants()
    assert c == dict(RS_TILE=ns.RS_TILE, CS_INLINE=ns.CS_INLINE, CS_WORK_CAP=ns.CS_WORK_CAP)
    assert [ns.digit_plan(1 << b) for b in (1, 8, 9, 10, 11, 16, 17, 18, 19, 20, 21, 24, 25, 27)] == \
        [(1, 8), (1, 8), (1, 9), (1, 10), (2, 8), (2, 8), (2, 9), (2, 9), (2, 10), (2, 10), (3, 8), (3, 8), (3, 9), (3, 9)]


PLAN_OF = {"bits04_one_clump": (4, (1, 8)), "bits08_2pow8": (8, (1, 8)), "bits09": (9, (1, 9)), "bits10_2pow10": (10, (1, 10)),
           "bits11_2pow10_plus_row": (11, (2, 8)), "bits16_2pow16": (16, (2, 8)), "bits17": (17, (2, 9)), "bits18_2pow18": (18, (2, 9)),
           "bits19": (19, (2, 10)), "bits20_2pow20": (20, (2, 10)), "bits21_above_2pow20": (21, (3, 8)), "bits24_2pow24": (24, (3, 8)),
           "bits25_above_2pow24": (25, (3, 9))}


@pytest.mark.parametrize("name", list(ns.PLAN_GRIDS))
def test_digit_plan_scenes(name):
    scene, grid, ci, lists = first_step(ns.plan_scene, name)
    bits, plan = PLAN_OF[name]
    assert grid == ns.PLAN_GRIDS[name]
    ncells = grid[0] * grid[1]
    assert ns.ilog2_ceil(ncells) == bits and ns.digit_plan(ncells) == plan
    assert ns.clumps_are_apart(scene) and len(np.unique(ci)) == 4 * len(scene["sites"])     # every clump in four cells of its own
    assert ci.min() == grid[0] + 1 and ci.max() == ncells - grid[0] - 2                 # both corners of the grid's interior are occupied
    assert len(ci) <= 2000
    assert_sets_are_brute_force(scene, lists)
    # every particle has a neighbour in another cell
    off, idx = lists
    rows = np.repeat(np.arange(len(ci)), np.diff(off.astype(np.int64)))
    assert (np.bincount(rows, weights=(ci[idx.astype(np.int64)] != ci[rows]), minlength=len(ci)) > 0).all()
    # ... and shuffled: the same sets under the other numbering
    sh = ns.shuffled(scene)
    _, sh_lists = oracle_steps(sh)
    assert_sets_are_brute_force(sh, sh_lists)


def test_digit_plan_scenes_cover_every_plan_at_both_ends():
    plans = {}
    for name, (sx, sy) in ns.PLAN_GRIDS.items():
        plans.setdefault(ns.digit_plan(sx * sy), []).append(ns.ilog2_ceil(sx * sy))
    assert sorted(plans) == sorted(ns.ALL_PLANS)
    # first and last bit count of each plan ((1, 8) from the smallest grid there is; (3, 9) ends at the grid limit, 27 bits: only its first)
    assert {p: (min(b), max(b)) for p, b in plans.items()} == {(1, 8): (4, 8), (1, 9): (9, 9), (1, 10): (10, 10), (2, 8): (11, 16), (2, 9): (17, 18),
                                                              (2, 10): (19, 20), (3, 8): (21, 24), (3, 9): (25, 25)}
    assert ns.PLAN_GRIDS["bits10_2pow10"] == (32, 32) and ns.PLAN_GRIDS["bits20_2pow20"] == (1024, 1024) and ns.PLAN_GRIDS["bits24_2pow24"] == (4096, 4096)
    # the second step's build is queued ahead on the grid + 2 cells on every side: a merge where that grid holds at most n + 4096 cells
    ahead = {name: (sx + 4) * (sy + 4) for name, (sx, sy) in ns.PLAN_GRIDS.items()}
    merged = [name for name in ns.PLAN_GRIDS if ahead[name] <= len(ns.plan_scene(name)["mass"]) + ns.MERGE_SLACK]
    assert merged == ["bits04_one_clump", "bits08_2pow8", "bits09", "bits10_2pow10", "bits11_2pow10_plus_row"]


@pytest.mark.parametrize("n", list(ns.EDGE_COUNTS))
def test_tile_edge_scenes(n):
    scene, grid, ci, lists = first_step(ns.edge_scene, n)
    assert len(ci) == n
    assert_sets_are_brute_force(scene, lists)
    tiles = (n + ns.RS_TILE - 1) // ns.RS_TILE
    assert tiles == (2 if n == 2049 else 1)
    assert (n < 64) == (n == 63)                                      # less than one wave of keys
    assert n % 1024 in (63, 64, 65, 1023, 0, 1) and n % ns.RS_TILE in (63, 64, 65, 1023, 1024, 1025, 2047, 0, 1)


def test_tile_and_trip_counts_of_the_large_lattices():
    """1025 x 1025: 514 tiles of 2048 keys -- a partial last tile (1 key) and, in k_rs_rowscan, a thread whose four counts end in
    mid-vector (514 = 4 x 128 + 2) inside the first trip; 1449 x 1449: 1026 tiles -- a second trip of two tiles."""
    for side, tiles, trips in ((1025, 514, 1), (1449, 1026, 2)):
        n = side * side
        assert (n + ns.RS_TILE - 1) // ns.RS_TILE == tiles and (tiles + ns.RS_TRIP - 1) // ns.RS_TRIP == trips
        assert tiles % 4 != 0 and n % ns.RS_TILE not in (0, ns.RS_TILE - 1)
    assert 1025 * 1025 % ns.RS_TILE == 1 and 1026 % ns.RS_TRIP == 2


def test_cell_table_scenes():
    scene, grid, ci, lists = first_step(ns.table_threshold_scene)
    gaps = ns.key_gaps(ci)
    assert ns.clumps_are_apart(scene)
    assert (gaps == ns.CS_INLINE - 1).sum() >= 50 and (gaps == ns.CS_INLINE).sum() >= 50 and (gaps == ns.CS_INLINE + 1).sum() >= 20
    assert 0 < (gaps >= ns.CS_INLINE).sum() < ns.CS_WORK_CAP
    assert_sets_are_brute_force(scene, lists)
    scene, grid, ci, lists = first_step(ns.table_overflow_scene)
    gaps = ns.key_gaps(ci)
    assert ns.clumps_are_apart(scene)
    assert (gaps >= ns.CS_INLINE).sum() > ns.CS_WORK_CAP + 5000          # the work list overflows by thousands of entries
    assert grid[0] < ns.GRID_DIM_LIMIT and 8e6 < grid[0] * grid[1] < 16e6 and ns.digit_plan(grid[0] * grid[1]) == (3, 8)
    assert len(ci) == 320760 and len(ci) + ns.MERGE_SLACK < grid[0] * grid[1]
    assert_sets_are_brute_force(scene, lists)


@pytest.mark.parametrize("transpose", [False, True])
def test_grid_limit_scenes(transpose):
    for length, fits in ((ns.LIMIT_FITS, True), (ns.LIMIT_REFUSED, False)):
        scene, grid, ci, lists = first_step(ns.limit_scene, length, transpose)
        assert grid == ((8, length) if transpose else (length, 8))
        assert (length < ns.GRID_DIM_LIMIT) == fits and 65000 <= ns.LIMIT_FITS
        # the largest cell coordinate along the strip uses all 16 bits; the grid queued ahead (+ 4) no longer fits either way
        cmax = (ci // grid[0] if transpose else ci % grid[0]).max()
        assert cmax == length - 2 and cmax >= 1 << 15 and length + 2 * ns.AHEAD_MARGIN >= ns.GRID_DIM_LIMIT
        assert ns.clumps_are_apart(scene)
        assert_sets_are_brute_force(scene, lists)


@pytest.mark.parametrize("name", list(ns.MULTIRES_SCENES))
def test_multiresolution_strips(name):
    extent, ratio, doublings, tile = ns.MULTIRES_SCENES[name]
    scene, grid, ci, lists = first_step(ns.two_size_strip, extent, ratio)
    coarse, fine, k, ts = ns.sorting_grid(scene["pos"], scene["mass"])
    assert coarse == grid and (k, ts) == (doublings, tile)
    h = ns.h_of_mass(scene["mass"])
    assert np.float32(h.max()) >= np.float32(1.75) * h.min()
    if name == "fine_grid_fits":
        assert fine[0] < ns.GRID_DIM_LIMIT and fine[0] > 3 * coarse[0]
    else:
        # the fine particles' own grid is too wide; what is sorted by is twice that cell (ratio 4) or the coarse grid itself (ratio 2)
        width_fine_cells = (scene["pos"][:, 0].max() - scene["pos"][:, 0].min()) / (2.0 * float(h.min()))
        assert width_fine_cells >= ns.GRID_DIM_LIMIT and (fine == coarse) == (name == "coarse_grid_only")
        assert fine[0] < ns.GRID_DIM_LIMIT and (name == "coarse_grid_only" or fine[0] > 1.9 * coarse[0])
    assert_sets_are_brute_force(scene, lists)
    # fine and coarse particles are on each other's lists
    off, idx = lists
    rows = np.repeat(np.arange(len(h)), np.diff(off.astype(np.int64)))
    assert (h[rows] != h[idx.astype(np.int64)]).sum() >= 20


@pytest.mark.parametrize("admitted", [True, False])
def test_merge_admission_scenes(admitted):
    scene = ns.two_blocks(ns.merge_gap_for(32, admitted))
    n = len(scene["mass"])
    steps, lists = oracle_steps(scene, ns.MERGE_STEPS, ns.forced_params(max_iters=3, max_dt=ns.MERGE_MAX_DT))
    for x, (sx, sy), ci in steps:
        reported, predicted = sx * sy, (sx + 2 * ns.AHEAD_MARGIN) * (sy + 2 * ns.AHEAD_MARGIN)
        if admitted:      # within three columns of the limit
            assert n <= reported and n + ns.MERGE_SLACK - 3 * (sy + 4) < predicted <= n + ns.MERGE_SLACK
        else:
            assert n + ns.MERGE_SLACK < reported < n + ns.MERGE_SLACK + 3 * sy and predicted > n + ns.MERGE_SLACK
    assert steps[0][1] == steps[-1][1]                                        # no edge crossed a cell boundary on the way
    moved = np.abs(steps[-1][0] - steps[0][0]).max()
    assert 1e-4 < moved < 0.1 * 2.0 * float(ns.h_of_mass(scene["mass"][0]))    # the blocks moved, by less than a tenth of a cell


# ------------------------------------------------------------------------------------------------
# the checkers bite
# ------------------------------------------------------------------------------------------------
class _Grid:
    def __init__(self, sx, sy):
        self.size_x, self.size_y = sx, sy


def test_the_order_check_and_the_set_check_bite():
    scene, (sx, sy), ci, lists = first_step(ns.table_threshold_scene)
    scene = ns.shuffled(scene)                      # (the defects below must show in an upload order that is not the cell order)
    steps, lists = oracle_steps(scene)
    ci = steps[0][2]
    grid, n = _Grid(sx, sy), len(ci)
    want = ns.brute_force_keys(scene)
    # the model of a correct build passes both checks
    off, idx = ns.model_device_lists(scene, grid, ci)
    assert np.array_equal(ns.csr_keys(off, idx), want) and ns.slot_order_violations(off, idx, ci) == 0
    # (the oracle's own lists are ascending in the host index, not in the slot: the order check is not vacuous)
    assert ns.slot_order_violations(*lists, ci) > 0
    # 1. an unstable sort: two particles of one cell change places -- the sets are unchanged, the order is not
    perm = np.argsort(ci, kind="stable")
    key = ci[perm]
    s = int(np.nonzero(key[1:] == key[:-1])[0][0])
    bad = perm.copy()
    bad[[s, s + 1]] = perm[[s + 1, s]]
    off, idx = ns.model_device_lists(scene, grid, ci, perm=bad)
    assert np.array_equal(ns.csr_keys(off, idx), want) and ns.slot_order_violations(off, idx, ci) > 0
    # 2. / 3. stale entries of the cell table (what a denser scene before left there, or zeros), one cell each
    table = ns.cell_table(ci, sx * sy)
    keys = np.unique(ci)
    g = int(np.nonzero(np.diff(keys) - 1 >= ns.CS_INLINE)[0][3])              # a long gap between occupied cells a < b of one row
    a, b = int(keys[g]), int(keys[g + 1])
    assert a // sx == b // sx
    for cell, stale, what in ((a + 1, 0, "first gap cell"), (b - 1, n, "last gap cell = one before an occupied cell"),
                              (b - 1, int(table[b]) + 1, "one before an occupied cell, off by one")):
        t = table.copy()
        assert t[cell] != stale
        t[cell] = stale
        off, idx = ns.model_device_lists(scene, grid, ci, table=t)
        assert not np.array_equal(ns.csr_keys(off, idx), want), what
    # (an entry in the middle of the gap is read by nobody: the model is the device's access pattern, not a table comparison)
    t = table.copy()
    t[(a + b) // 2] = n
    off, idx = ns.model_device_lists(scene, grid, ci, table=t)
    assert np.array_equal(ns.csr_keys(off, idx), want)
