"""BASELINE.json configs[3] (2D dam-break, 8 388 608 particles = configs[1]'s column eight times as wide, slab decomposition) and configs[4] (ratio-stress scene,
4 004 343 particles at 50:1 radii, IISPH, Sdf2D box, EmptyAngle level estimation) at FULL size, through the C ABI.

configs[3]: against the CPU oracle (bit-exact cell / neighbour indices, positions and densities within 1e-4 after N steps with
the iteration counts forced equal), and the 8-slab decomposition (loopback transport: 8 contexts of this process on one GPU,
the driver code the RCCL transport runs) against the single context.
configs[4]: the step path of the scene against the oracle at full size -- the oracle enumerates candidates with one grid
per size class (oracle/neigh.c), so 50:1 at 4M particles takes seconds per step, not hours.  The scene's host-side adaptivity
(split / merge / share) is exercised by tests/test_gpu_adaptivity.py.
"""
import numpy as np
import pytest

from adaptive_sph_amd import distributed as D, ffi, scene as sc
from adaptive_sph_amd.workloads import WORKLOADS
from tests.oracle_harness import displacement_bars, same_sets

pytestmark = pytest.mark.gpu

REL_TOL_FIELDS = 1e-4     # north_star: fp32 positions / densities within 1e-4 relative after N steps
FORCED = dict(hybrid_dfsph_max_avg_density_error=0.0, hybrid_dfsph_max_avg_divergence_error=0.0, iisph_max_avg_density_error=0.0)


def rel_err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    s = np.abs(b).max()
    return np.abs(a - b).max() / (s if s > 0 else 1.0)


def make_pair(product_lib, oracle_lib, name, **overrides):
    scene_f, params_f, _ = WORKLOADS[name]
    scn, P = scene_f(), params_f(**overrides)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    g, o = ffi.Context(product_lib, len(mass), planes), ffi.Context(oracle_lib, len(mass), planes)
    g.upload(mass, pos, vel)
    o.upload(mass, pos, vel)
    g.pos0 = pos
    return g, o, P


def assert_displacements(g, o):
    ok, rep = displacement_bars(g.download("position"), o.download("position"), g.pos0)
    assert ok, rep


CONFIG3 = [("dam_break_8m", 8388608, 3), ("dam_break_8m_spec", 8386816, 8)]
"""configs[3] twice: round 4's eight-configs[1]-columns scene (8192 x 1024 at spacing 1/1024, 1 024-row halos) and SURVEY.md section 8d's
geometry AS WRITTEN (simulation.rs:2915-2983 add_fluid_block: pos [-1.9995, -0.9995], size [1.4143, 1.4143], spacing 1/2048 ->
2896 x 2896, box 4 x 2; max_dt 0.00025, profiles/r5_config3_divergence.md) -- the scene bench.py quotes as `strong_8m_spec`, with
2 896-row halos on eight slabs (VERDICT r5 missing 3 / next 1a).  Third entry: steps against the oracle -- at max_dt 0.00025 three steps
move a particle 19 ulp of its coordinate, which the displacement bars refuse as "not meaningful"; eight steps move it > 100."""


@pytest.mark.parametrize("name,n_expected,steps", CONFIG3)
def test_config3_dam_break_8m_against_the_oracle(product_lib, oracle_lib, name, n_expected, steps):
    g, o, P = make_pair(product_lib, oracle_lib, name, max_iters=3, **FORCED)
    assert g.n == n_expected
    p = P.to_ffi()
    for s in range(steps):
        sg, so = g.step(p), o.step(p)
        assert abs(sg.dt - so.dt) <= 1e-6 * so.dt, s
        assert sg.div_solver.iters == so.div_solver.iters and sg.density_solver.iters == so.density_solver.iters
    gg, og = g.grid(), o.grid()
    assert (gg.cell_size, gg.cells_min_x, gg.cells_min_y, gg.size_x, gg.size_y) == \
           (og.cell_size, og.cells_min_x, og.cells_min_y, og.size_x, og.size_y)
    for f in ("h2", "cell_index", "neighbor_count", "lambda_sum"):
        assert np.array_equal(g.download(f), o.download(f)), f
    same_sets(g, o)
    for f in ("position", "density", "aii", "ppe_source_term"):
        assert rel_err(g.download(f), o.download(f)) < REL_TOL_FIELDS, f
    assert rel_err(g.download("velocity"), o.download("velocity")) < 1e-3     # carries the unconverged (3 iterations) pressure field
    assert_displacements(g, o)


@pytest.mark.parametrize("name,n_expected,steps", CONFIG3)
def test_config3_dam_break_8m_eight_slabs_against_the_single_context(product_lib, name, n_expected, steps):
    scene_f, params_f, _ = WORKLOADS[name]
    scn, P = scene_f(), params_f(max_iters=3, **FORCED)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    p = P.to_ffi()
    single = ffi.Context(product_lib, len(mass), planes)
    single.upload(mass, pos, vel)
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 8)
    assert sum(c.n for c in grp) == len(mass) == n_expected and min(c.n for c in grp) > 1000000
    for s in range(steps):
        st1 = single.step(p)
        sts = ffi.group_step(grp, p)
        assert all(st.dt == st1.dt for st in sts)
        assert all(st.div_solver.iters == st1.div_solver.iters and st.density_solver.iters == st1.density_solver.iters for st in sts)
    n = len(mass)
    ids = np.concatenate([c.download("particle_id") for c in grp])
    assert np.array_equal(np.sort(ids), np.arange(n))                              # nothing lost or duplicated
    assert np.array_equal(D.gather_by_id(grp, "neighbor_count", n), single.download("neighbor_count"))
    for f, tol in (("position", 1e-5), ("velocity", 1e-4), ("density", 1e-5), ("mass", 0.0)):
        assert rel_err(D.gather_by_id(grp, f, n), single.download(f)) <= tol, f
    # (a position bar of 1e-5 of max|x| is ~100 ulp of a coordinate: more than the first steps move a particle -- the displacement
    #  from the uploaded positions is the bar that can fail)
    ok, rep = displacement_bars(D.gather_by_id(grp, "position", n), single.download("position"), pos)
    assert ok, rep
    st = grp[3].dist_get_stats()
    assert st["n_ghost"][0] > 0 and st["n_ghost"][1] > 0 and st["exchanges"] > 0    # an inner slab has two neighbours
    # the slabs' neighbour lists (global ids, ghosts included) are the single context's ENTRY BY ENTRY (this test
    # compared counts, sums and sums of squares until round 5): (row = global particle id, neighbour id) packed into one 64-bit key per
    # entry, sorted, compared whole -- 109 M entries over the eight slabs
    so, si = single.download_neighbors()
    cnt_ref = np.diff(so.astype(np.int64))
    key_ref = (np.repeat(np.arange(n, dtype=np.uint64), cnt_ref) << np.uint64(32)) | si.astype(np.uint64)
    del si
    key_ref.sort()
    keys = []
    for c in grp:
        pid = c.download("particle_id")
        off, idx = c.download_neighbors()
        assert np.array_equal(np.diff(off.astype(np.int64)), cnt_ref[pid])
        keys.append((np.repeat(pid.astype(np.uint64), np.diff(off.astype(np.int64))) << np.uint64(32)) | idx.astype(np.uint64))
        del off, idx
    key_grp = np.concatenate(keys)
    del keys
    key_grp.sort()
    assert np.array_equal(key_grp, key_ref)


def test_config4_ratio_stress_4m_step_path_on_eight_slabs(product_lib):
    """BASELINE configs[4]'s scene (4 002 768 fine + 1 575 coarse particles, 50:1 radii, IISPH, Sdf2D box, EmptyAngle level estimation)
    on the EIGHT x-slabs BASELINE.json names, against the single context.  The ghost layer of a cut is as wide as the largest
    smoothing length NEAR THAT CUT demands (sph_context.hpp: Dist::hcut) -- seven of the eight slabs are 0.069-wide slices of the
    fine block, a fifth of the ghost layer the coarse particles' support would ask for, which round 3 refused beyond two slabs."""
    scene_f, params_f, _ = WORKLOADS["ratio_stress_4m"]
    scn, P = scene_f(), params_f(level_estimation_method="EmptyAngle", max_iters=3, **FORCED)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    p = P.to_ffi()
    single = ffi.Context(product_lib, len(mass), planes)
    single.upload(mass, pos, vel)
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 8)
    assert sum(c.n for c in grp) == len(mass) and min(c.n for c in grp) > 400000
    for s in range(3):
        st1 = single.step(p)
        sts = ffi.group_step(grp, p)
        assert all(st.dt == st1.dt for st in sts)
        assert all(st.density_solver.iters == st1.density_solver.iters for st in sts)
    n = len(mass)
    ids = np.concatenate([c.download("particle_id") for c in grp])
    assert np.array_equal(np.sort(ids), np.arange(n))
    assert np.array_equal(D.gather_by_id(grp, "neighbor_count", n), single.download("neighbor_count"))
    for f, tol in (("position", 1e-5), ("velocity", 1e-4), ("density", 1e-5), ("mass", 0.0), ("level_estimation", 1e-4)):
        assert rel_err(D.gather_by_id(grp, f, n), single.download(f)) <= tol, f
    # the inner slabs of the fine block carry ghost layers of a few thousand particles, not the 660 k a global-width layer held
    st = grp[3].dist_get_stats()
    assert 0 < st["n_ghost"][0] < 100000 and 0 < st["n_ghost"][1] < 100000, st
    for c in grp:
        c.close()
    single.close()


def test_config3_dam_break_8m_eight_ranks_on_their_own_threads(product_lib):
    """configs[3] the way 8 processes would run it: 8 slab contexts, one host thread each, every rank calling sph_step by itself
    (thread transport: the per-rank driver code with its rank-local branches; a collective not entered by all or an unmatched
    send is an error).  Bit for bit the loopback group's result."""
    scene_f, params_f, _ = WORKLOADS["dam_break_8m"]
    scn, P = scene_f(), params_f(max_iters=3, **FORCED)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    p = P.to_ffi()
    loop = D.make_loopback_group(product_lib, pos, mass, vel, planes, 8)
    thr = D.ThreadedGroup(product_lib, pos, mass, vel, planes, 8)
    try:
        for s in range(3):
            a = ffi.group_step(loop, p)
            b = thr.step(p)
            assert all(x.dt == y.dt and x.div_solver.iters == y.div_solver.iters for x, y in zip(a, b))
        for ca, cb in zip(loop, thr.contexts):
            assert ca.n == cb.n > 1000000
            for f in ("particle_id", "position", "density", "neighbor_count"):
                assert np.array_equal(ca.download(f), cb.download(f)), f
        st = thr.contexts[4].dist_get_stats()
        assert st["n_ghost"][0] > 0 and st["n_ghost"][1] > 0 and st["bytes_sent"] > 0
    finally:
        thr.close()


def test_config4_ratio_stress_4m_against_the_oracle(product_lib, oracle_lib):
    """The step path of configs[4] with the recipe's own parameters (media/ratio-stress-test-video.yaml: IISPH, cfl 0.2,
    AnalyticUnderestimate = the Sdf2D box) and default-config.yaml's EmptyAngle level estimation, iteration counts pinned."""
    g, o, P = make_pair(product_lib, oracle_lib, "ratio_stress_4m", level_estimation_method="EmptyAngle", max_iters=3, **FORCED)
    assert g.n == 4002768 + 1575
    p = P.to_ffi()
    for s in range(2):
        sg, so = g.step(p), o.step(p)
        assert abs(sg.dt - so.dt) <= 1e-6 * so.dt, s
    h = o.download("h2")
    assert 49.9 < h.max() / h.min() < 50.1                                         # the 50:1 radius ratio is the scene's purpose
    gg, og = g.grid(), o.grid()
    assert (gg.cell_size, gg.cells_min_x, gg.cells_min_y, gg.size_x, gg.size_y) == \
           (og.cell_size, og.cells_min_x, og.cells_min_y, og.size_x, og.size_y)
    for f in ("h2", "cell_index", "neighbor_count", "lambda_sum", "flag_is_fluid_surface", "flag_insufficient_neighs"):
        assert np.array_equal(g.download(f), o.download(f)), f
    same_sets(g, o)
    assert 0 < o.download("flag_is_fluid_surface").sum() < g.n
    for f in ("position", "density", "aii", "ppe_source_term", "velocity"):
        assert rel_err(g.download(f), o.download(f)) < REL_TOL_FIELDS, f
    assert_displacements(g, o)
    for f in ("level_estimation", "level_old"):
        a, b = g.download(f), o.download(f)
        assert np.array_equal(np.isnan(a), np.isnan(b)), f
        assert float(np.nanmax(np.abs(a - b))) / max(float(np.nanmax(np.abs(b))), 1e-30) < REL_TOL_FIELDS, f
    g.classify(p), o.classify(p)
    cg, co = g.download("particle_size_class"), o.download("particle_size_class")
    assert (cg != co).mean() < 1e-3
    # 4M fine particles far from the 1575 coarse ones: 3 x 3 stencils of the fine grid, row masks (sph_list_forms)
    forms = g.profile_list_forms()
    assert forms["n_lists"] == g.n and forms["n_mask"] >= 0.9 * g.n and forms["n_walk"] == 0, forms


def test_config4_ratio_stress_4m_blocks_in_contact(product_lib, oracle_lib):
    """The same scene with the fine block moved against the coarse one: a coarse particle then has thousands of fine
    neighbours (beyond every recorded-list form: it walks its candidates in each sweep), a fine particle at the interface a
    stencil dozens of cells wide.  Sets bit-exact, fields within tolerance."""
    scene_f, params_f, _ = WORKLOADS["ratio_stress_4m"]
    scn, P = scene_f(), params_f(max_iters=3, **FORCED)
    scn.blocks[1].pos[0] = 0.4 - 0.55 - 0.0004385 * 20       # fine block's right edge ~one coarse spacing left of the coarse block
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    g, o = ffi.Context(product_lib, len(mass), planes), ffi.Context(oracle_lib, len(mass), planes)
    g.upload(mass, pos, vel)
    o.upload(mass, pos, vel)
    p = P.to_ffi()
    for s in range(3):
        sg, so = g.step(p), o.step(p)
        assert abs(sg.dt - so.dt) <= 1e-5 * so.dt, s
    cnt = o.download("neighbor_count")
    assert cnt.max() > 2000 and (cnt > 128).sum() >= 60        # the coarse block's 63 interface particles, buried in fine neighbours: beyond every recorded-list form
    assert np.array_equal(g.download("neighbor_count"), cnt)
    assert np.array_equal(g.download("cell_index"), o.download("cell_index"))
    same_sets(g, o)
    for f in ("position", "density", "aii"):
        assert rel_err(g.download(f), o.download(f)) < REL_TOL_FIELDS, f
    ok, rep = displacement_bars(g.download("position"), o.download("position"), pos)
    assert ok, rep


def test_config4_settled_blocks_against_the_oracle(product_lib, oracle_lib):
    """configs[4] under load (VERDICT r4 missing 4 / next 6; profiles/r5_config4_settled.md): the scene's two blocks standing on the floor
    (`scene.ratio_stress_4m_settled`), the recipe's IISPH parameters, steps 0..7 with the iteration count forced to 6.  The lattice
    starts 7 % short of rho_0 and closes up under gravity: from step 6 on the solve works on POSITIVE pressures (the free-falling
    reference scene never does: test_config4_ratio_stress_4m_against_the_oracle; the 50:1 interface: ..._blocks_in_contact).  Sets entry
    by entry, fields within north_star's tolerance."""
    g, o, P = make_pair(product_lib, oracle_lib, "ratio_stress_4m_settled", max_iters=6, **FORCED)
    assert g.n == 4002768 + 1575
    p = P.to_ffi()
    for s in range(8):
        sg, so = g.step(p), o.step(p)
        assert abs(sg.dt - so.dt) <= 1e-5 * so.dt, s
        assert int(sg.density_solver.iters) == int(so.density_solver.iters), s      # (0 while every pressure is clamped: n_normal == 0 ends the solve)
    assert int(so.density_solver.iters) == 6
    for f in ("h2", "cell_index", "neighbor_count", "lambda_sum"):
        assert np.array_equal(g.download(f), o.download(f)), f
    same_sets(g, o)
    # the last solve worked on positive pressures, on both sides alike
    assert so.density_solver.normal_count > 1000, int(so.density_solver.normal_count)
    assert abs(int(sg.density_solver.normal_count) - int(so.density_solver.normal_count)) <= 0.02 * so.density_solver.normal_count + 10
    assert (o.download("pressure") > 0).sum() > 1000
    for f in ("position", "density", "aii", "ppe_source_term"):
        assert rel_err(g.download(f), o.download(f)) < REL_TOL_FIELDS, f
    assert rel_err(g.download("velocity"), o.download("velocity")) < 1e-3      # v += dt a^p of the unconverged iterate (see TOL in test_gpu_parity)
    assert rel_err(g.download("pressure"), o.download("pressure")) < 2e-3
    assert_displacements(g, o)


def test_config2_columns_in_contact_at_full_size(product_lib, oracle_lib):
    """configs[2] with the two resolutions IN CONTACT (VERDICT r5 missing 4 / next 1b; sph_kernels.rs:273-278, SURVEY 8d item 3:
    "exercises the symmetric (h_i + h_j) / 2 neighbour rule once the two columns collide").  BASELINE's placement starts the blocks 2.0
    apart -- they meet after thousands of steps, so neither test_full_size_parity_adaptive_4to1_against_the_oracle (3 steps) nor the
    free-standing bench leg ever evaluates a mixed-h pair.  Here the same two blocks -- 942 080 fine + 58 880 coarse particles, 4:1 radii
    -- stand one COARSE spacing apart (`scene.dam_break_1m_adaptive_contact`): every fine particle within a coarse support of the
    interface has a stencil wider than 3 x 3 cells of the fine sorting grid and records an explicit index list, a coarse interface
    particle dozens of fine neighbours.  (Free-running this placement blows up at step 5 -- density solve at max_iters, 1e26 m/s -- on the
    recipe's own parameters: profiles/r6_config2_contact.md; with forced counts it is a parity scene, the bench leg takes the blocks 1.5
    coarse spacings apart, which collide dynamically.)  3 steps, iteration counts forced; sets entry by entry, fields within north_star's 1e-4."""
    g, o, P = make_pair(product_lib, oracle_lib, "dam_break_1m_adaptive_contact", max_iters=3, **FORCED)
    assert g.n == 942080 + 58880
    p = P.to_ffi()
    for s in range(3):
        sg, so = g.step(p), o.step(p)
        assert abs(sg.dt - so.dt) <= 1e-6 * so.dt, s
        assert sg.div_solver.iters == so.div_solver.iters and sg.density_solver.iters == so.density_solver.iters
    h = o.download("h2")
    assert 3.99 < h.max() / h.min() < 4.01
    gg, og = g.grid(), o.grid()
    assert (gg.cell_size, gg.cells_min_x, gg.cells_min_y, gg.size_x, gg.size_y) == \
           (og.cell_size, og.cells_min_x, og.cells_min_y, og.size_x, og.size_y)
    for f in ("h2", "cell_index", "neighbor_count", "lambda_sum"):
        assert np.array_equal(g.download(f), o.download(f)), f
    same_sets(g, o)
    # the interface is there: mixed-h pairs on both sides of it
    off, idx = o.download_neighbors()
    cnt = np.diff(off.astype(np.int64))
    mass = o.download("mass")
    fine = mass < mass.max() * 0.5
    row_fine = np.repeat(fine, cnt)
    mixed = row_fine != fine[idx]
    n_mixed_rows_fine = len(np.unique(np.repeat(np.arange(g.n), cnt)[mixed & row_fine]))
    n_mixed_rows_coarse = len(np.unique(np.repeat(np.arange(g.n), cnt)[mixed & ~row_fine]))
    # (measured: 1 609 fine particles -- the last two fine columns, 920 rows -- and 230 coarse ones -- the first coarse column -- carry mixed-h pairs)
    assert n_mixed_rows_fine > 1500 and n_mixed_rows_coarse >= 200, (n_mixed_rows_fine, n_mixed_rows_coarse)
    del off, idx, row_fine, mixed
    # ... and the device works it on explicit index lists (or candidate walks) -- every particle with a mixed-h pair and, the stencil width
    # being decided per tile of the sorting grid, the fine particles around them --, the bulk on row masks
    forms = g.profile_list_forms()
    assert forms["n_lists"] == g.n and forms["n_index"] + forms["n_walk"] >= n_mixed_rows_fine + n_mixed_rows_coarse and forms["n_mask"] > 0.9 * g.n, forms
    print("config2 in contact: list forms", forms, "mixed rows", n_mixed_rows_fine, n_mixed_rows_coarse)
    for f in ("position", "density", "aii", "ppe_source_term"):
        assert rel_err(g.download(f), o.download(f)) < REL_TOL_FIELDS, f
    assert rel_err(g.download("velocity"), o.download("velocity")) < 1e-3     # carries the unconverged (3 iterations) pressure field
    assert_displacements(g, o)
