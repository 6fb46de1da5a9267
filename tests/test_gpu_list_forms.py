"""Every neighbour-list FORM against the CPU oracle, at the thresholds where the density (BUILD) sweep switches between them
(adaptive_sph_amd/csrc/sph_sweeps.hip: mask word <= 32 candidates per row; 16-bit offset list <= 24 others, every j - i within int16; explicit
index list <= 128 entries where index lists are recorded; the candidate walk otherwise; SPH_ERR_TOO_MANY_NEIGHBORS above 20 000).

The form of every particle is PREDICTED on the host (tests/oracle_harness.py: predict_list_forms, from the oracle's cells and neighbour
counts) and profile_list_forms() must EQUAL the prediction, so "this scene walks" is an asserted fact; what each scene has to exercise
(LIST_FORM_REQUIREMENTS: a form's share >= 20 % and >= 500 particles, rows of exactly 32 and 33 candidates, lists of 24 / 25 others and of
128 / 129 entries, waves that hold two forms, wall terms in the outermost occupied columns and rows) is asserted beside it and, without a
device, in tests/test_list_form_predictor.py.  The sorting grid keeps one empty cell around the particles, so no particle ever sits in
column 0 / sx - 1: the outermost occupied cells are the ones whose candidate ranges begin and end exactly at sweep_particle's clamps.
(A squeeze of 0.66 of the 48 x 40 block is not among the scenes: it predicts 410 walk lanes, below the floor of 500, and lists of at most 29.)

Which off-by-one of a threshold comparison each test is built to catch:
  * `(re[dr] - rb[dr]) <= 32u` -> `<= 33u` (ok_list): test_forms_neighbour_sets_and_first_sweeps[rows_32_33-*] -- n_mask / n_walk differ
    from the prediction by the particles with a 33-candidate row (and their 33rd candidate has no mask bit: neighbour sets, density);
  * `rec_idx && nacc <= NLX_CAP` -> `< NLX_CAP` (NL_IDX): test_forms_neighbour_sets_and_first_sweeps[index_128_129-exact] -- n_index /
    n_walk differ by the particles with exactly 128 entries;
  * `d >= -32768` -> `d >= -32769` (emit_offset_list): test_strip_offset_lists_at_the_16_bit_limit -- the strip holds lanes whose smallest difference is exactly
    -32769 and whose largest is exactly +32768 (assert_strip_crossings); with the mutation such a lane would replay offset +32767 for a
    neighbour 32769 slots below: not bit-identical to the mask replay, and off the oracle.
The first two are confirmed on the host, where the same off-by-one applied to the predictor changes the predicted counts of these scenes
(tests/test_list_form_predictor.py::test_an_off_by_one_threshold_changes_the_predicted_counts); the kernels themselves were not rebuilt
with the mutations.
"""
import numpy as np
import pytest

from adaptive_sph_amd import ffi, scene as sc
from adaptive_sph_amd.workloads import dam_break_params
from tests import oracle_harness as oh
from tests import test_gpu_bitexact as bitexact
from tests import test_gpu_parity as parity
from tests.oracle_harness import displacement_bars, same_sets

pytestmark = pytest.mark.gpu

SCENES = sorted(oh.LIST_FORM_SCENES)
SOLVERS = ["HybridDFSPH", "IISPH", "OnlyDivergence", "IISPH2"]
SQUEEZED = dict(max_dt=2e-5, max_iters=4)   # a squeezed lattice bursts apart: short steps, forced counts, the first steps only
TRAJECTORY_FIELDS = ["velocity", "density", "ppe_source_term", "pressure", "pressure_accel"]
REFERENCE_FACTOR = 8.0   # == parity.WINDOW_P99_RHO_FACTOR: device-vs-oracle over oracle-vs-oracle in another summation order


def forced(**kw):
    return parity.forced(**{**SQUEEZED, **kw})


def pair(glib, oracle_lib, scn, pos, mass, vel, policy="fast"):
    planes = sc.boundary_planes(scn.boundary)
    g, o = ffi.Context(glib, len(mass), planes), ffi.Context(oracle_lib, len(mass), planes)
    if policy != "fast":
        g.set_math_policy(policy)
    g.upload(mass, pos, vel)
    o.upload(mass, pos, vel)
    return g, o


def assert_lists_match(g, o):
    gg, og = g.grid(), o.grid()
    assert (gg.cell_size, gg.cells_min_x, gg.cells_min_y, gg.size_x, gg.size_y) == (og.cell_size, og.cells_min_x, og.cells_min_y, og.size_x, og.size_y)
    for f in ("h2", "cell_index", "neighbor_count", "lambda_sum"):
        assert np.array_equal(g.download(f), o.download(f)), f
    same_sets(g, o)


def lane_errors(a, b, lanes):
    """largest |a - b| over `lanes`, relative to the field's largest magnitude over ALL particles (parity.rel_err's scale)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b)[lanes].max()) / max(float(np.abs(b).max()), 1e-300)


@pytest.mark.parametrize("policy", ["fast", "exact"])
@pytest.mark.parametrize("name", SCENES)
def test_forms_neighbour_sets_and_first_sweeps(product_lib, oracle_lib, name, policy):
    """First step from identical inputs.  The device's form counts EQUAL the host prediction; cells, h, neighbour counts, wall terms and
    the neighbour sets entry by entry equal the oracle's; and the single sweeps (density, constant field, a_ii) meet the project's sweep
    bar on the walk lanes and on the mask lanes apart (FAST: a crowded uniform lane really walks; EXACT: it records an index list up to
    128 entries and walks beyond)."""
    scn, pos, mass, vel = oh.LIST_FORM_SCENES[name]()
    g, o = pair(product_lib, oracle_lib, scn, pos, mass, vel, policy)
    p = forced().to_ffi()
    sg, so = g.step(p), o.step(p)
    assert sg.dt == so.dt
    facts = oh.list_form_facts(o, pos, policy)
    assert oh.LIST_FORM_REQUIREMENTS[name][policy](facts), {k: v for k, v in facts.items() if not isinstance(v, np.ndarray)}
    measured = g.profile_list_forms()
    print(name, policy, "forms", measured, "predicted", facts["counts"])
    assert measured == facts["counts"]
    assert_lists_match(g, o)
    form = facts["form"]
    crowded, plain = form != oh.FORM_MASK, form == oh.FORM_MASK
    for f in parity.SWEEP_FIELDS:
        a, b = g.download(f), o.download(f)
        e_crowded = lane_errors(a, b, crowded)
        e_plain = lane_errors(a, b, plain) if plain.any() else None
        print(name, policy, f, "crowded lanes", e_crowded, "mask lanes", e_plain)
        assert e_crowded < parity.REL_TOL_SWEEP, (f, e_crowded)
        if e_plain is not None:
            assert e_plain < parity.REL_TOL_SWEEP, (f, e_plain)
            if policy == "fast" and plain.sum() >= 500:
                # The same pairs in the same slot order: a walk that is systematically a little off shows as a multiple of the mask lanes'
                # error (both relative to the field's largest magnitude, parity.rel_err's scale; floor: one f32 rounding, for a field the
                # mask lanes reproduce exactly).  The oracle against itself in another upload order (cell order, reversed, shuffled; CPU)
                # gives walk / mask = 0.43 .. 1.67 over density, constant_field and a_ii in half_squeezed and squeeze_0.60, the two scenes
                # with >= 500 mask lanes: the ratio is stable there, so 4 x holds as a bar.
                print(name, policy, f, "walk / mask", e_crowded / max(e_plain, 1e-300))
                assert e_crowded <= 4.0 * max(e_plain, float(np.finfo(np.float32).eps)), (f, e_crowded, e_plain)
    g.close()
    o.close()


@pytest.fixture
def exact(monkeypatch):
    monkeypatch.setenv("SPH_HIP_EXACT", "1")   # read by sph_create


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", ["squeeze_0.55", "half_squeezed", "index_128_129", "corners"])
def test_crowded_lanes_bit_for_bit_under_exact(product_lib, oracle_lib, exact, name, solver):
    """EXACT policy, upload in the device's visiting order, a fresh upload from the oracle's state every step (tests/test_gpu_bitexact.py):
    tolerance 0 on every field and on the residual classes.  Crowded rows record index lists (squeeze_0.55, half_squeezed, corners);
    index_128_129 holds lists of 128 entries (index list) and 129 (candidate walk) side by side."""
    scn, pos, mass, vel = oh.LIST_FORM_SCENES[name]()
    bitexact.stepwise(product_lib, oracle_lib, mass, pos, vel, sc.boundary_planes(scn.boundary), bitexact.forced(pressure_solver_method=solver, **SQUEEZED), 2)


# The reference against ITSELF: the oracle on the same particles uploaded in another order (reversed, the device's cell order, a seeded
# shuffle; the largest of the three) against the oracle in host order, 3 forced steps of max_dt = 2e-5 / max_iters = 4, measured on the CPU
# by reference_sensitivity() below (python -m tests.test_gpu_list_forms prints this table).  Per scene and solver: parity.rel_err of
# velocity, density, ppe_source_term, pressure, pressure_accel, then the displacement error relative to the displacement (the larger of the
# max and the median figure of displacement_bars).  A squeezed block is badly conditioned -- IISPH2 throws particles out at 1e7 m/s -- so
# the bar of a trajectory field is max(the project's bar, 8 x this), never anything the device produced.
REFERENCE_SENSITIVITY = {
    ("corners", "HybridDFSPH"): [0.00083, 0.0004, 0.0014, 0.00054, 0.00083, 0.00052],
    ("corners", "IISPH"): [0.001, 0.00056, 0.0013, 0.00027, 0.001, 0.00066],
    ("corners", "OnlyDivergence"): [9.3e-07, 8.3e-07, 1.2e-06, 1.6e-06, 1.2e-06, 0.0],
    ("corners", "IISPH2"): [0.026, 0.00018, 0.00018, 0.0048, 0.026, 0.027],
    ("half_squeezed", "HybridDFSPH"): [0.00024, 7.7e-05, 0.00016, 9.8e-05, 0.00022, 0.00013],
    ("half_squeezed", "IISPH"): [0.00037, 5.5e-05, 0.00024, 0.00017, 0.00036, 0.00018],
    ("half_squeezed", "OnlyDivergence"): [1.6e-07, 3.8e-07, 1.2e-06, 4e-06, 1.2e-06, 0.0],
    ("half_squeezed", "IISPH2"): [0.0021, 0.00012, 0.00015, 0.00097, 0.0021, 0.0022],
    ("index_128_129", "HybridDFSPH"): [0.011, 0.00025, 0.027, 0.016, 0.013, 0.0062],
    ("index_128_129", "IISPH"): [0.013, 0.00025, 0.032, 0.016, 0.013, 0.0062],
    ("index_128_129", "OnlyDivergence"): [1.1e-06, 1e-06, 1e-06, 1.6e-06, 1.1e-06, 0.0],
    ("index_128_129", "IISPH2"): [0.00039, 0.00014, 0.00014, 0.00034, 0.00039, 0.00035],
    ("rows_32_33", "HybridDFSPH"): [0.0004, 6.1e-05, 0.00021, 0.00017, 0.00039, 0.00024],
    ("rows_32_33", "IISPH"): [0.00034, 8.3e-05, 0.00013, 3.6e-05, 0.0003, 0.00015],
    ("rows_32_33", "OnlyDivergence"): [9e-08, 4.8e-07, 2e-06, 6.4e-06, 3.9e-06, 0.0],
    ("rows_32_33", "IISPH2"): [0.00019, 7.6e-05, 8.8e-05, 3e-05, 0.00019, 0.0002],
    ("squeeze_0.45", "HybridDFSPH"): [0.00075, 0.00041, 0.0014, 0.0004, 0.00075, 0.00047],
    ("squeeze_0.45", "IISPH"): [0.0012, 0.00037, 0.0013, 0.0002, 0.0011, 0.00073],
    ("squeeze_0.45", "OnlyDivergence"): [9.3e-07, 7.3e-07, 1.4e-06, 1.1e-06, 1.2e-06, 0.0],
    ("squeeze_0.45", "IISPH2"): [0.013, 0.00015, 0.00015, 0.0048, 0.013, 0.013],
    ("squeeze_0.55", "HybridDFSPH"): [0.00084, 0.00017, 0.00017, 0.00023, 0.00079, 0.00055],
    ("squeeze_0.55", "IISPH"): [0.00065, 0.0002, 0.00039, 0.00041, 0.00059, 0.0004],
    ("squeeze_0.55", "OnlyDivergence"): [1.8e-07, 4.7e-07, 2.5e-06, 8.2e-06, 4.1e-06, 0.0],
    ("squeeze_0.55", "IISPH2"): [0.00042, 0.00012, 0.00015, 0.00022, 0.00042, 0.00043],
    ("squeeze_0.60", "HybridDFSPH"): [0.00018, 2.8e-05, 6e-05, 0.00013, 0.00019, 0.00011],
    ("squeeze_0.60", "IISPH"): [9.1e-05, 2.8e-05, 0.0001, 0.00012, 8.7e-05, 7.4e-05],
    ("squeeze_0.60", "OnlyDivergence"): [9.2e-08, 5.5e-07, 1.9e-06, 5.3e-06, 3.5e-06, 0.0],
    ("squeeze_0.60", "IISPH2"): [0.0011, 0.00013, 0.00016, 0.0013, 0.0011, 0.0013],
}


def reference_sensitivity(oracle_lib, name, solver, steps=3):
    scn, pos, mass, vel = oh.LIST_FORM_SCENES[name]()
    planes = sc.boundary_planes(scn.boundary)
    p = forced(pressure_solver_method=solver).to_ffi()

    def run(order):
        o = ffi.Context(oracle_lib, len(mass), planes)
        o.upload(mass[order], pos[order], vel[order])
        for _ in range(steps):
            o.step(p)
        inv = np.argsort(order)
        out = {f: o.download(f)[inv] for f in TRAJECTORY_FIELDS + ["position"]}
        o.close()
        return out

    n = len(mass)
    base = run(np.arange(n))
    worst = np.zeros(len(TRAJECTORY_FIELDS) + 1)
    for order in (np.arange(n)[::-1].copy(), bitexact.device_order(pos, bitexact.h_from_mass(mass)), np.random.default_rng(1).permutation(n)):
        other = run(order)
        figs = [parity.rel_err(other[f], base[f]) for f in TRAJECTORY_FIELDS]
        _, rep = displacement_bars(other["position"], base["position"], pos)
        figs.append(max(rep["max_err"] / max(rep["max_disp"], 1e-300), rep["median_err"] / max(rep["median_disp"], 1e-300)) if rep["max_disp"] > 50 * rep["ulp"] else 0.0)
        worst = np.maximum(worst, figs)
    return [float("%.2g" % v) for v in worst]


def assert_positions(g, o, pos0, rel, where):
    """displacement_bars; where the ORACLE's particles moved by less than rounding (OnlyDivergence from rest, one short step of the strip
    whose coordinates reach 126: g dt^2 is below one ulp of a coordinate) the positions agree to that ulp instead"""
    ok, rep = displacement_bars(g.download("position"), o.download("position"), pos0, rel)
    print(where, "displacement", rep)
    if rep["max_disp"] <= 50 * rep["ulp"]:
        assert rep["max_err"] <= rep["ulp"], (where, rep)
    else:
        assert ok, (where, rep)


def assert_dt(sg, so, s, sens, where):
    """dt: identical inputs on the first step, so equal to the bit.  From the second step on these scenes are CFL-limited (dt ~ 1e-6, far
    below max_dt): dt is a constant over the largest speed, and so carries the relative error of the velocity field -- its bar."""
    if s == 0:
        assert sg.dt == so.dt, where
    else:
        bar = max(parity.REL_TOL_FIELDS, REFERENCE_FACTOR * sens[0])
        print(where, "step", s, "dt", sg.dt, so.dt, "bar", bar)
        assert abs(sg.dt - so.dt) <= bar * so.dt, (where, s, sg.dt, so.dt)


def assert_trajectory(g, o, pos0, sens, where):
    for k, f in enumerate(TRAJECTORY_FIELDS):
        bar = max(parity.TOL.get(f, parity.REL_TOL_FIELDS), REFERENCE_FACTOR * sens[k])
        err = parity.rel_err(g.download(f), o.download(f))
        print(where, f, err, "bar", bar)
        assert err < bar, (where, f, err, bar)
    assert_positions(g, o, pos0, max(1e-3, REFERENCE_FACTOR * sens[-1]), where)


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", SCENES)
def test_three_forced_steps_under_fast(product_lib, oracle_lib, name, solver):
    """The whole step, the product's default policy, 3 forced-count steps with crowded lanes walking their candidates in every sweep."""
    scn, pos, mass, vel = oh.LIST_FORM_SCENES[name]()
    g, o = pair(product_lib, oracle_lib, scn, pos, mass, vel)
    p = forced(pressure_solver_method=solver).to_ffi()
    for s in range(3):
        sg, so = g.step(p), o.step(p)
        assert_dt(sg, so, s, REFERENCE_SENSITIVITY[(name, solver)], f"{name} {solver}:")
        if s == 0:
            assert g.profile_list_forms()["n_walk"] == oh.list_form_facts(o, pos)["counts"]["n_walk"] >= 500
            # identical inputs: the project's own bars, without the sensitivity term
            for f in TRAJECTORY_FIELDS:
                err = parity.rel_err(g.download(f), o.download(f))
                print(name, solver, "first step", f, err)
                assert err < parity.TOL.get(f, parity.REL_TOL_FIELDS), (name, solver, f, err)
    assert_trajectory(g, o, pos, REFERENCE_SENSITIVITY[(name, solver)], f"{name} {solver}:")
    g.close()
    o.close()


# squeeze_0.45, EmptyAngle, 3 forced steps: level_estimation / level_old of the oracle uploaded in reversed order against the oracle in
# host order (relative to the largest distance; surface flags and NaN patterns identical), measured on the CPU
LEVEL_SENSITIVITY_SQUEEZE_045 = 1.7e-4


def test_level_estimation_on_crowded_extended_lists(product_lib, oracle_lib):
    """EmptyAngle before advection on squeeze_0.45: the extended-range lists (5.5 / 1.9 of the support) pass 128 entries, index list ->
    candidate walk, in the detection, propagation and smoothing sweeps."""
    scn, pos, mass, vel = oh.LIST_FORM_SCENES["squeeze_0.45"]()
    g, o = pair(product_lib, oracle_lib, scn, pos, mass, vel)
    p = forced(level_estimation_method="EmptyAngle", maximum_surface_distance=0.2, particle_radius_fine=0.004, particle_radius_base=0.02).to_ffi()
    for s in range(3):
        sg, so = g.step(p), o.step(p)
        assert_dt(sg, so, s, REFERENCE_SENSITIVITY[("squeeze_0.45", "HybridDFSPH")], "squeeze_0.45 EmptyAngle:")
        fg, fo = g.download("flag_is_fluid_surface"), o.download("flag_is_fluid_surface")
        assert 0 < fo.sum() < len(fo) and np.array_equal(fg, fo), f"step {s}: {(fg != fo).sum()} surface flags differ"
        assert np.array_equal(g.download("flag_insufficient_neighs"), o.download("flag_insufficient_neighs"))
        for f in ("level_estimation", "level_old", "stash"):   # parity._level_fields_match with the bar of this scene
            a, b = g.download(f), o.download(f)
            assert np.array_equal(np.isnan(a), np.isnan(b)), (s, f)
            err = float(np.nanmax(np.abs(a - b))) / max(float(np.nanmax(np.abs(b))), 1e-30) if not np.isnan(b).all() else 0.0
            print("squeeze_0.45 EmptyAngle step", s, f, err)
            assert err < max(parity.REL_TOL_FIELDS, REFERENCE_FACTOR * LEVEL_SENSITIVITY_SQUEEZE_045), (s, f, err)
    assert_trajectory(g, o, pos, REFERENCE_SENSITIVITY[("squeeze_0.45", "HybridDFSPH")], "squeeze_0.45 EmptyAngle:")
    g.close()
    o.close()


def test_free_running_counts_with_mixed_waves(product_lib, oracle_lib):
    """half_squeezed with the stop tolerances of the dam break (no forced counts): the stop decisions of the two Jacobi loops within +-1
    of the oracle's (tests/test_gpu_parity.py::test_free_running_iteration_counts).  On this block the damped Jacobi iteration does not
    converge -- with the default cap of 200 iterations the ORACLE's pressures overflow in the first step (SPH_ERR_AP_NOT_FINITE) -- so the
    cap is 20, and the steps compared are the first three: the oracle against itself in another upload order (reversed, shuffled; CPU)
    gives the same counts there, (2, 20), (3, 20), (20, 20), and counts 2 apart from the fourth step on (5 / 7, 20 / 18), where dt has
    fallen to 2e-10 and the block has burst.  The divergence loop stops on its tolerance in the first two steps, not on the cap."""
    scn, pos, mass, vel = oh.LIST_FORM_SCENES["half_squeezed"]()
    g, o = pair(product_lib, oracle_lib, scn, pos, mass, vel)
    p = dam_break_params(max_dt=2e-5, max_iters=20).to_ffi()
    diffs, counts = [], []
    for s in range(3):
        sg, so = g.step(p), o.step(p)
        counts.append((int(so.div_solver.iters), int(so.density_solver.iters), int(sg.div_solver.iters), int(sg.density_solver.iters)))
        diffs.append(max(abs(counts[-1][0] - counts[-1][2]), abs(counts[-1][1] - counts[-1][3])))
    print("free-running (oracle div, density, device div, density)", counts)
    assert max(diffs) <= 1, counts
    assert all(1 < c[0] < 20 for c in counts[:2]), counts   # (stopped by the tolerance)
    g.close()
    o.close()


@pytest.mark.parametrize("solver", ["HybridDFSPH", "IISPH"])
def test_strip_offset_lists_at_the_16_bit_limit(lab_lib, oracle_lib, monkeypatch, solver):
    """strip_scene: 15 800 x 6 particles in three cell rows of 15 800 / 47 400 / 31 600, every lane with a mask word and at most 24
    others -- only the 16-bit range of j - i decides between offset list and mask word, and the strip crosses +32767 (bottom row, middle
    of the strip) and -32768 (top row, near its right end): assert_strip_crossings.  The laboratory build with offset lists (the default)
    against SPH_OFFSET_LISTS=0 bit for bit over free-running steps, and the default against the oracle."""
    scn = oh.strip_scene()
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    p = forced(pressure_solver_method=solver).to_ffi()
    o = ffi.Context(oracle_lib, len(mass), planes)
    o.upload(mass, pos, vel)
    o.step(p)
    facts = oh.list_form_facts(o, pos)
    print("strip crossings at columns", oh.assert_strip_crossings(facts, pos, o.grid(), o.download("cell_index")))
    free = dam_break_params(pressure_solver_method=solver, max_dt=0.0005).to_ffi()
    out = {}
    for form in ("offsets", "masks"):
        if form == "masks":
            monkeypatch.setenv("SPH_OFFSET_LISTS", "0")
        g = ffi.Context(lab_lib, len(mass), planes)   # (the switches are read at sph_create)
        if form == "masks":
            monkeypatch.delenv("SPH_OFFSET_LISTS")
        g.upload(mass, pos, vel)
        st = g.step(p)
        if form == "offsets":   # the forced first step against the oracle
            assert g.profile_list_forms() == facts["counts"]
            assert_lists_match(g, o)
            for f in parity.SWEEP_FIELDS:
                for lanes, what in ((facts["has_list"], "offset lists"), (~facts["has_list"], "mask words")):
                    e = lane_errors(g.download(f), o.download(f), lanes)
                    print("strip", solver, f, what, e)
                    assert e < parity.REL_TOL_SWEEP, (f, what, e)
            for f in ("ppe_source_term", "pressure", "pressure_accel", "velocity"):
                assert parity.rel_err(g.download(f), o.download(f)) < parity.TOL.get(f, parity.REL_TOL_FIELDS), f
            assert_positions(g, o, pos, 1e-3, f"strip {solver}:")
        its, fields = [], []
        for _ in range(5):
            st = g.step(free)
            its.append((int(st.div_solver.iters), int(st.density_solver.iters), int(st.density_solver.normal_count),
                        np.float32(st.density_solver.avg_error).view(np.uint32).item(), np.float32(st.dt).view(np.uint32).item()))
            fields.append({f: g.download(f) for f in ("position", "velocity", "pressure", "density", "neighbor_count", "aii", "constant_field")})
        out[form] = (its, fields)
        g.close()
    o.close()
    assert out["offsets"][0] == out["masks"][0]
    for s, (fa, fb) in enumerate(zip(out["offsets"][1], out["masks"][1])):
        for f in fa:
            assert np.array_equal(fa[f], fb[f]), (s, f)


@pytest.mark.parametrize("policy", ["fast", "exact"])
def test_neighbour_count_guard_at_20000(product_lib, oracle_lib, policy):
    """cluster_scene: one particle inside a circle of equal ones, all within its support.  With 19 999 others its list holds exactly
    20 000 entries, self included: both sides step, counts and sets equal.  With 20 000 others it holds 20 001: both sides return
    SPH_ERR_TOO_MANY_NEIGHBORS (16) -- a status of the library, no device fault -- the context is poisoned, and an upload of a sane scene
    clears that and steps to the oracle's result.
    Why a 20 001-entry row writes nothing out of bounds (read in sph_sweeps.hip): the walk (walk_row) only READS candidates b <= j < e
    of the cell table's ranges; under FAST a crowded uniform lane records nothing but its three 32-bit masks (`bit < 32u` guards the
    shift); under EXACT IdxRecorder::push stores group nacc >> 2 only while nacc < NLX_CAP = 128, flush likewise, so the last group
    written is 31 = NLX_GROUPS - 1 whatever the row holds, and the count kept in the list word is masked to 16 bits (20 001 < 65 536)."""
    planes = sc.boundary_planes(sc.SceneBoundary("box", 4.0, 2.0))
    p = forced().to_ffi()
    pos, mass, vel = oh.cluster_scene(oh.MAX_NEIGHBOR_COUNT - 1)
    g, o = ffi.Context(product_lib, len(mass) + 1, planes), ffi.Context(oracle_lib, len(mass) + 1, planes)
    if policy != "fast":
        g.set_math_policy(policy)
    g.upload(mass, pos, vel)
    o.upload(mass, pos, vel)
    sg, so = g.step(p), o.step(p)
    assert sg.dt == so.dt
    nc = o.download("neighbor_count")
    assert nc.max() == nc[0] == oh.MAX_NEIGHBOR_COUNT
    assert np.array_equal(g.download("neighbor_count"), nc)
    assert np.array_equal(g.download("cell_index"), o.download("cell_index"))
    # 137 M list entries: equal CSR offsets, equal per-particle sums of the indices and of their squares, and the sets entry by entry for
    # the centre and 64 sampled ring particles (same_sets' 64-bit key sort over all of them would dominate the module's run time)
    go, gi = g.download_neighbors()
    oo, oi = o.download_neighbors()
    assert np.array_equal(go, oo)
    starts = go[:-1].astype(np.int64)
    for power in (1, 2):
        assert np.array_equal(np.add.reduceat(gi.astype(np.uint64) ** power, starts), np.add.reduceat(oi.astype(np.uint64) ** power, starts)), power
    for i in [0] + list(np.random.default_rng(0).integers(1, len(mass), 64)):
        assert np.array_equal(np.sort(gi[go[i]:go[i + 1]]), oi[oo[i]:oo[i + 1]]), i
    del gi, oi
    forms = g.profile_list_forms()
    assert forms["n_walk"] >= 1 and forms["n_mask"] == 0, forms   # every row here holds thousands of candidates
    # one particle more
    pos, mass, vel = oh.cluster_scene(oh.MAX_NEIGHBOR_COUNT)
    g.upload(mass, pos, vel)
    o.upload(mass, pos, vel)
    for ctx in (o, g):
        with pytest.raises(ffi.SphError) as e:
            ctx.step(p)
        assert e.value.status == 16, e.value
    with pytest.raises(ffi.SphError) as e:
        g.step(p)
    assert e.value.status == 31   # SPH_ERR_POISONED until the next upload
    scn, pos, mass, vel = oh.squeezed_scene(1.0)
    g.upload(mass, pos, vel)
    o.upload(mass, pos, vel)
    q = parity.forced(max_iters=4).to_ffi()
    sg, so = g.step(q), o.step(q)
    assert sg.dt == so.dt
    assert_lists_match(g, o)
    for f in parity.SWEEP_FIELDS:
        assert parity.rel_err(g.download(f), o.download(f)) < parity.REL_TOL_SWEEP, f
    g.close()
    o.close()


if __name__ == "__main__":   # the table above, from the CPU oracle alone
    lib = oh.load_oracle()
    for nm in SCENES:
        for sv in SOLVERS:
            print(f'    ("{nm}", "{sv}"): {reference_sensitivity(lib, nm, sv)},', flush=True)
