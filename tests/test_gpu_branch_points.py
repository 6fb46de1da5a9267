"""The step at the branch points of its wall and pair distances (scenes: tests/branch_point_scenes.py; what they hold and that the oracle
stays inside its bars on them: tests/test_branch_point_scenes.py, on the CPU).

  1. EXACT policy: the oracle bit for bit with particles at d <= -1, in (-1, 0], exactly on -1, -0.5, 0 and beside them, behind two
     walls at once; with pairs at r = 0, inside and just outside the gradient's cut-off; with pairs on the edge of the support.
  2. FAST policy against the dense f64 restatement.  On the close pairs the restatement is evaluated twice, with the reference's cut-off
     (grad W = 0 for q <= 1e-5) and without it: FAST keeps no cut-off, and may differ from the reference by what that explains, no more.
  3. The neighbour sets under FAST with pairs one f32 step inside, on and outside the edge, and pairs a contracted r2 would flip.
  4. The record and offset forms against their generic twins over 12 steps with wall-flagged particles behind the wall and duplicates.
  5. The level estimation on the same scenes."""
import numpy as np
import pytest

from adaptive_sph_amd import ffi
from tests import branch_point_scenes as B
from tests.neighbour_scenes import csr_keys
from tests.oracle_harness import load_oracle
from tests.test_branch_point_scenes import keys_of_sets
from tests.test_gpu_bitexact import STEP_FIELDS, exact, stepwise   # noqa: F401  (exact: the fixture)
from tests.test_oracle_independent import _compare, compare_level_on, dense_step

pytestmark = pytest.mark.gpu

LEVEL = dict(level_estimation_method="EmptyAngle", maximum_surface_distance=0.2)
LEVEL_FIELDS = STEP_FIELDS + ["level_estimation", "flag_is_fluid_surface", "flag_insufficient_neighs", "stash"]


def run_stepwise(product_lib, oracle_lib, s, P, steps, fields=STEP_FIELDS):
    stepwise(product_lib, oracle_lib, s["mass"], s["pos"], s["vel"], s["planes"], P, steps, fields)


# ---- 1. EXACT is the oracle bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("handler", ["AnalyticOverestimate", "AnalyticUnderestimate"])
@pytest.mark.parametrize("pen", B.PENALTIES)
def test_wall_depths_penalties_and_handlers_bit_for_bit(product_lib, oracle_lib, exact, pen, handler):
    s = B.wall_depths(handler)
    run_stepwise(product_lib, oracle_lib, s, B.case_params(3, boundary_penalty_term=pen, init_boundary_handler=handler), 2)


@pytest.mark.parametrize("solver,kw", [("IISPH", {}), ("IISPH2", {}), ("HybridDFSPH", dict(operator_discretization="ConsistentSimpleGradient")),
                                       ("HybridDFSPH", dict(operator_discretization="Winchenbach2020")),
                                       ("IISPH", dict(operator_discretization="Winchenbach2020", two_sizes=True)),
                                       ("HybridDFSPH", dict(two_sizes=True, pen="Quadratic2"))])
def test_wall_depths_solvers_and_discretisations_bit_for_bit(product_lib, oracle_lib, exact, solver, kw):
    """(the wall term of the divergence and the corner's two entries differ per discretisation; the third one refuses this scene: below)"""
    kw = dict(kw)
    s = B.wall_depths(two_sizes=kw.pop("two_sizes", False))
    run_stepwise(product_lib, oracle_lib, s, B.case_params(3, solver, boundary_penalty_term=kw.pop("pen", "Quadratic1"), **kw), 2)


CLOSE_EXACT = [(solver, two, {}) for solver in ("HybridDFSPH", "IISPH", "OnlyDivergence", "IISPH2") for two in (False, True)] + \
              [("HybridDFSPH", k % 2 == 1, dict(operator_discretization=op, viscosity_type=visc, viscosity=0.01))
               for k, (op, visc) in enumerate((op, visc) for op in ("ConsistentSimpleGradient", "ConsistentSymmetricGradient", "Winchenbach2020")
                                              for visc in ("ApproxLaplace", "WCSPH"))]


@pytest.mark.parametrize("solver,two_sizes,kw", CLOSE_EXACT)
def test_close_pairs_bit_for_bit(product_lib, oracle_lib, exact, solver, two_sizes, kw):
    run_stepwise(product_lib, oracle_lib, B.close_pairs(two_sizes), B.case_params(3, solver, **kw), 2)


@pytest.mark.parametrize("policy", ["fast", "exact"])
def test_wall_depths_symmetric_gradient_is_refused_as_the_reference_refuses_it(product_lib, oracle_lib, monkeypatch, policy):
    """ConsistentSymmetricGradient takes p_ib = p_i at the walls, and behind a wall the closed form of a_ii turns negative: the reference
    asserts (simulation.rs:1390-1403), and so do the oracle and the device -- the same sign from the same wall terms"""
    if policy == "exact":
        monkeypatch.setenv("SPH_HIP_EXACT", "1")
    s = B.wall_depths()
    p = B.case_params(3, operator_discretization="ConsistentSymmetricGradient").to_ffi()
    for lib in (product_lib, oracle_lib):
        c = ffi.Context(lib, len(s["mass"]), s["planes"])
        c.upload(s["mass"], s["pos"], s["vel"])
        with pytest.raises(ffi.SphError, match="SPH_ERR_AII_NEGATIVE|AII should not be negative"):
            c.step(p)
        c.close()


@pytest.mark.parametrize("two_sizes", [False, True])
def test_support_edge_bit_for_bit(product_lib, oracle_lib, exact, two_sizes):
    run_stepwise(product_lib, oracle_lib, B.support_edge(2.0, two_sizes), B.case_params(3), 1)


# ---- 2. FAST against the dense f64 restatement ------------------------------------------------------------------------------------
def assert_begin_is_the_oracles(g, s, P):
    """OpDensity::begin is IEEE in every policy: the wall sums, h and the counts equal the oracle's bit for bit; everything finite"""
    o = ffi.Context(load_oracle(), len(s["mass"]), s["planes"])
    o.upload(s["mass"], s["pos"], s["vel"])
    o.step(P.to_ffi())
    for f in ("lambda_sum", "lambda_grad_sum", "h2", "neighbor_count"):
        assert np.array_equal(g.download(f), o.download(f)), f
    o.close()
    for f in STEP_FIELDS:
        assert np.isfinite(g.download(f).astype(np.float64)).all(), f


@pytest.mark.parametrize("pen,two_sizes", [(pen, False) for pen in B.PENALTIES] + [("Quadratic2", True)])
def test_wall_depths_fast_against_dense_f64(product_lib, pen, two_sizes):
    s = B.wall_depths(two_sizes=two_sizes)
    P = B.case_params(3, boundary_penalty_term=pen)
    g = ffi.Context(product_lib, len(s["mass"]), s["planes"])
    _compare(g, s["pos"], s["mass"], s["vel"], P, 3, 10.0, s["box"], block=False)
    assert (g.download("lambda_sum") >= 1.0).sum() >= 20          # (particles at d <= -1 did step)
    assert_begin_is_the_oracles(g, s, P)
    g.close()


# today's FAST bars (tests/test_oracle_independent.py: _compare at tol = 10), per field of the step
FAST_BARS = dict(density=2e-5, aii=5e-5, ppe_source_term=5e-5, pressure=1e-4, pressure_accel=1e-4, velocity=1e-4, position=2e-4)


@pytest.mark.parametrize("solver,max_iters,two_sizes", [("IISPH", 0, False), ("IISPH", 3, False), ("HybridDFSPH", 3, False), ("HybridDFSPH", 3, True),
                                                        ("IISPH", 3, True)])
def test_close_pairs_fast_is_within_what_the_missing_cutoff_explains(product_lib, solver, max_iters, two_sizes):
    """The restatement with the reference's cut-off (A) and without it (B); FAST has none between q = 3e-8 and 1e-5.
       per field      max |FAST - A| <= today's bar x max |A| + max |B - A|
       per particle   |FAST - A|_i   <= today's bar x max |A| + 1.05 |B - A|_i
       per field      max |FAST - B| <= today's bar x max |A|
    a_ii is a sum over the particle's own pairs: a particle with no partner inside the band gets today's bar alone there (the other
    fields carry the band pairs' difference on through the solve).  Velocity and position as the step's change, as in _compare."""
    s = B.close_pairs(two_sizes)
    P = B.case_params(max_iters, solver)
    L = load_oracle().lib
    g = ffi.Context(product_lib, len(s["mass"]), s["planes"])
    g.upload(s["mass"], s["pos"], s["vel"])
    st = g.step(P.to_ffi())
    assert st.density_solver.iters == max_iters
    lam, dlam = (lambda d: float(L.oracle_lambda2(d))), (lambda d: float(L.oracle_dlambda2(d)))
    a = dense_step(s["pos"], s["mass"], s["vel"], P, float(st.dt), max_iters + 1, (), lam, dlam)
    b = dense_step(s["pos"], s["mass"], s["vel"], P, float(st.dt), max_iters + 1, (), lam, dlam, cutoff=None)
    cq = B.close_partners(s)
    in_band = (cq >= B.Q_FAST_ZERO) & (cq <= B.Q_CUTOFF)
    assert in_band.sum() >= 24 and (np.isfinite(cq) & ~in_band).sum() >= 60
    assert np.array_equal(g.download("neighbor_count"), a["neighbor_count"])
    report = {}
    for f, bar in FAST_BARS.items():
        got, fa, fb = g.download(f).astype(np.float64), a[f], b[f]
        assert np.isfinite(got).all(), f
        if f in ("velocity", "position"):
            start = s["vel" if f == "velocity" else "pos"].astype(np.float64)
            got, fa, fb = got - start, fa - start, fb - start
        rows = lambda x: np.abs(x).reshape(len(x), -1).max(axis=1)   # noqa: E731
        err, gap = rows(got - fa), rows(fb - fa)
        floor = bar * np.abs(fa).max() + (1.2e-7 if f == "position" else 0.0)
        report[f] = (gap.max() / np.abs(fa).max(), err.max() / np.abs(fa).max(), rows(got - fb).max() / np.abs(fa).max())
        print(f"close_pairs {solver} {max_iters} two_sizes={two_sizes} {f}: cut-off gap {report[f][0]:.3g}, FAST against the cut-off {report[f][1]:.3g}, "
              f"against none {report[f][2]:.3g} (of the max-norm)")
        assert err.max() <= floor + gap.max(), (f, report[f])
        assert rows(got - fb).max() <= floor, (f, report[f])      # ... and it IS the arithmetic without the cut-off, to today's bar
        worst = int(np.argmax(err - 1.05 * gap))
        assert (err <= floor + 1.05 * gap).all(), (f, worst, err[worst], gap[worst], floor)
        if f == "aii":
            assert (err[~in_band] <= floor).all(), (f, float(err[~in_band].max()), floor)
    # the deviation is there to be bounded: without the cut-off the reference's own numbers move by more than its rounding
    assert report["pressure_accel"][0] > 3e-6, report
    g.close()


# ---- 3. neighbour sets under FAST on the edge of the support ------------------------------------------------------------------------
@pytest.mark.parametrize("two_sizes", [False, True], ids=["uniform_mask_words", "two_sizes_index_lists"])
def test_support_edge_sets_under_fast(product_lib, oracle_lib, two_sizes):
    s = B.support_edge(2.0, two_sizes)
    p = B.case_params(3).to_ffi()
    g, o = ffi.Context(product_lib, len(s["mass"]), s["planes"]), ffi.Context(oracle_lib, len(s["mass"]), s["planes"])
    for c in (g, o):
        c.upload(s["mass"], s["pos"], s["vel"])
        c.step(p)
    (go, gi), (oo, oi) = g.download_neighbors(), o.download_neighbors()
    assert np.array_equal(go, oo)
    want = keys_of_sets(B.f32_neighbour_sets(s["pos"], s["mass"], 2.0))
    assert np.array_equal(csr_keys(oo, oi), want) and np.array_equal(csr_keys(go, gi), want)
    assert np.array_equal(g.download("neighbor_count"), np.diff(go.astype(np.int64)))
    forms = g.profile_list_forms()
    print("support_edge two_sizes =", two_sizes, forms)
    g.close()
    o.close()


@pytest.mark.parametrize("two_sizes", [False, True])
@pytest.mark.parametrize("policy", ["fast", "exact"])
def test_support_edge_of_the_extended_lists(product_lib, oracle_lib, policy, two_sizes):
    """EmptyAngle before advection: the lists of range level_estimation_range / 1.9 live inside the step.  The flags and the stash
    against the oracle; and the host of every clump has two or three entries with the pair on the edge, so `fewer than 3` IS the pair's
    predicate: r2 == s2 and the value above it insufficient, the value below it not."""
    s = B.support_edge(B.k_extended(), two_sizes, clumps=True)
    p = B.case_params(2, **LEVEL).to_ffi()
    g, o = ffi.Context(product_lib, len(s["mass"]), s["planes"]), ffi.Context(oracle_lib, len(s["mass"]), s["planes"])
    g.set_math_policy(policy)
    for c in (g, o):
        c.upload(s["mass"], s["pos"], s["vel"])
        c.step(p)
    flag = g.download("flag_insufficient_neighs").astype(bool)
    assert [bool(flag[a]) for a, _, _, _ in s["clumps"]] == [kind != "below" for _, _, _, kind in s["clumps"]]
    assert np.array_equal(flag, o.download("flag_insufficient_neighs").astype(bool))
    assert np.array_equal(g.download("flag_is_fluid_surface"), o.download("flag_is_fluid_surface"))
    sg, so = g.download("stash"), o.download("stash")
    assert np.array_equal(np.isnan(sg), np.isnan(so))
    assert np.nanmax(np.abs(sg - so)) <= 2e-5 * np.nanmax(np.abs(so))      # (_compare_level's bar at tol = 10)
    (go, gi), (oo, oi) = g.download_neighbors(), o.download_neighbors()      # filtered down to the support again: k = 2
    assert np.array_equal(csr_keys(go, gi), csr_keys(oo, oi))
    g.close()
    o.close()


# ---- 4. record and offset forms against their generic twins ------------------------------------------------------------------------
RECORD_FIELDS = ("aii", "constant_field", "velocity", "position", "density", "pressure", "pressure_accel", "ppe_source_term", "lambda_sum")
COUNT = "aii_nonpressure_records"


@pytest.mark.parametrize("env", [dict(SPH_FUSE_RECORDS="0"), dict(SPH_ACCEL_GENERIC="1", SPH_JACOBI_GENERIC="1", SPH_SOURCE_GENERIC="1"),
                                 dict(SPH_ACCEL_GENERIC="1", SPH_SOURCE_GENERIC="1"), dict(SPH_OFFSET_LISTS="0")],
                         ids=["fuse_records_off", "generic_sweeps", "generic_accel_and_source", "offset_lists_off"])
def test_record_and_offset_forms_with_wall_flags_and_duplicates(lab_lib, monkeypatch, env):
    """wall_records, 12 steps, two contexts side by side: the default against one of its generic twins, every field and the lists bit for
    bit after every step; the record form of the fused sweep from step 1 on, with wall-flagged particles behind the wall and a list longer
    than an offset list in a record step.

    generic_sweeps found that SPH_JACOBI_GENERIC=1 was no twin of OpJacobiU (the other two switches are, alone or together): OpJacobiU sums
    gscale x e over the neighbours and multiplies the sum by m_i / rho_i once, OpJacobi multiplies every pair by m_j x v_rcp(rho_i) inside
    the fma -- equal coefficients for equal masses, other roundings.  Measured at step 0 (HybridDFSPH, 3 iterations): pressure differed in
    96 of 1042 particles by 1.2e-7 of its max-norm, a^p in 264 by 3.3e-7, velocity in 459 by 2.9e-7; nothing with one iteration (p = 0
    going in); the same without the duplicates or the wall shift.  The laboratory build now runs that switch through OpJacobiG
    (sph_sweeps.hip): OpJacobi's gathers, OpJacobiU's arithmetic.  The product's sweeps are unchanged."""
    s = B.wall_records()
    p = B.wall_records_params().to_ffi()
    pair = []
    for form in ("default", "twin"):          # (the switches are read at sph_create)
        for k, v in (env.items() if form == "twin" else ()):
            monkeypatch.setenv(k, v)
        c = ffi.Context(lab_lib, len(s["mass"]), s["planes"])
        for k in (env if form == "twin" else ()):
            monkeypatch.delenv(k)
        c.upload(s["mass"], s["pos"], s["vel"])
        c.profile_enable(1)
        pair.append(c)
    a, b = pair
    launches = lambda c: c.profile_get().get(COUNT, (0, 0))[0]   # noqa: E731
    forms, longest, behind = [], [], []
    for step in range(B.RECORD_STEPS):
        before, x = launches(a), a.download("position")      # (the wall terms of a step belong to the positions it starts from)
        sa, sb = a.step(p), b.step(p)
        assert (np.float32(sa.dt).view(np.uint32), int(sa.div_solver.iters), int(sa.density_solver.iters)) == \
               (np.float32(sb.dt).view(np.uint32), int(sb.div_solver.iters), int(sb.density_solver.iters)), step
        for f in RECORD_FIELDS:
            assert np.array_equal(a.download(f).view(np.uint32), b.download(f).view(np.uint32)), (step, f)
        (oa, ia), (ob, ib) = a.download_neighbors(), b.download_neighbors()
        assert np.array_equal(oa, ob) and np.array_equal(ia, ib), step
        forms.append(launches(a) - before)
        longest.append(int(np.diff(oa.astype(np.int64)).max()) - 1)
        behind.append(int(((x[:, 0] <= -2.0) & (a.download("lambda_sum") != 0)).sum()))
    print(env, "record form", forms, "longest list", longest, "wall-flagged behind the wall", behind)
    assert forms[0] == 0 and all(f == 1 for f in forms[1:]), forms          # the record form from step 1 on
    if "SPH_FUSE_RECORDS" in env:
        assert launches(b) == 0
    assert min(behind[:2]) >= 20, behind                                      # d <= 0 with wall terms, in a record step too
    assert any(f == 1 and n > B.NLOFF_SLOTS for f, n in zip(forms, longest)), (forms, longest)
    a.close()
    b.close()


# ---- 5. level estimation -----------------------------------------------------------------------------------------------------------
SCENES = {"close_pairs": B.close_pairs, "close_pairs_two_sizes": lambda: B.close_pairs(True), "wall_depths": B.wall_depths}


@pytest.mark.parametrize("scene", list(SCENES))
def test_level_estimation_bit_for_bit_on_branch_scenes(product_lib, oracle_lib, exact, scene):
    run_stepwise(product_lib, oracle_lib, SCENES[scene](), B.case_params(2, **LEVEL), 1, LEVEL_FIELDS)


@pytest.mark.parametrize("stash_mode", ["SurfaceDistanceFirstIteration", "SurfaceDistanceMiddle"])
@pytest.mark.parametrize("scene", list(SCENES))
def test_level_estimation_fast_against_dense_restatement_on_branch_scenes(product_lib, scene, stash_mode):
    s = SCENES[scene]()
    g = ffi.Context(product_lib, len(s["mass"]), s["planes"])
    compare_level_on(g, s["pos"], s["mass"], s["vel"], B.case_params(2, **LEVEL), s["planes"], stash_mode, 10.0, scene == "wall_depths", block=False)
    g.close()
