"""The FREE-RUNNING pressure solve: the residual sum the device reduces in its own fixed order, and the stop decision it takes from it.

Every other GPU test forces the iteration counts (tolerances 0, max_iters = K: the rule's only live branch is iter == max_iters) or
compares free-running counts with slack.  Here the device's reduction is predicted TO THE BIT by tests/solve_reference.py -- a numpy
float32 restatement of solver_block_partial (DPP network per wave, waves in index order), of solver_reduce_decide (strided partials per
thread, shuffle tree, waves in index order) and of solver_stop_rule -- fed with the CPU oracle's per-particle residuals, which the
EXACT policy reproduces bit for bit when both sides receive the particles in the device's visiting order (tests/test_gpu_bitexact.py).

  (a) forced K in {0, 1, 2, 5}: density_error is the oracle's to the bit; the device's counts and the bits of avg_error and max_error are
      the model's (density residual from the field density_error and the classes of a_ii / the final pressure; divergence residual
      dt (s - a_p), which no field keeps, from the oracle's own entry point oracle_solve_residuals).
  (b) the decision at its threshold: the two ADJACENT float32 tolerances whose thresholds bracket the model's value of iteration K
      (solve_reference.bracketing_tolerances; asserted on the CPU by tests/test_solve_reference.py): with the lower one the free solve
      (max_iters = 50) does not stop at K, with the upper one it stops exactly there and every field is the oracle's forced-K step.
      K = 2 (the first iteration the rule may stop at) and K = 5 (the model shows that iterations 2 .. 4 do not pass).  A huge tolerance
      stops at exactly 2 (iter > 1); all particles singular stop at 0 with a NaN average; max_iters = 32768 (> PROG_MAX_ITERS: the
      predicted queue, not the paced solve) decides the same.  The other solve of HybridDFSPH is stopped at iteration 2 on both sides by a
      huge tolerance, so that one max_iters can force the solve under test on the oracle.
  (c) the predicted free-running count K* in 4 .. 10 over three consecutive steps, tolerances recorded in solve_reference.FREE_CASES.
  (d) the same reduction behind the default (FAST) policy's sweep B -- records + offset lists on a uniform scene, the generic sweep on a
      two-size scene: the oracle is not bit-identical there and the reduction is a stage of its own, so the model is fed the DEVICE's
      downloaded density_error, a_ii and pressure.
  (e) slab groups of two and three ranks (loopback, and three ranks on threads).  A rank's slot layout with its ghosts is not exposed, so there is NO bit model of the per-rank
      sums here; pinned instead: every rank (an empty slab among them) reports the same iters and the same bits of avg_error, and the
      threshold pair built around the group's OWN forced-K value flips the count on all ranks together -- also where sweep A runs in two
      launches and k_solver_progress decides between them (DECIDE_NOT_HERE).

Sizes (solve_reference.SCENES): 56 (one wave), 575 (= 63 mod 64: the tail wave one lane short, 3 blocks), 1600 (= 6 * 256 + 64: one full
wave and three idle ones in the last block; 7 blocks, not a multiple of 8), 2809 (11 blocks: per_xcd = 2, the first size at which the logical
block is not the hardware's block index), 262 656 = 513 x 512 (1026 partials: the second trip of
solver_reduce_decide's strided loop, with 2 partials; the oracle steps it in ~0.5 s, so it was not shrunk; IISPH only, one step).  The
lattices are drawn together by 5 % (SQUEEZE) so that "normal" particles -- and with them nonzero partials -- fill the whole array.
"""
import numpy as np
import pytest

from adaptive_sph_amd import distributed as D
from adaptive_sph_amd import ffi, scene as sc
from adaptive_sph_amd.workloads import dam_break_params
from tests import solve_reference as R
from tests.solve_reference import device_order, h_from_mass
from tests.test_gpu_bitexact import STEP_FIELDS, assert_bit_identical, forced

pytestmark = pytest.mark.gpu
F = np.float32
FIELDS = STEP_FIELDS + ["density_error"]
_STATE = {}


def bits(x):
    return int(np.asarray(x, F).view(np.uint32))


def state(name):
    if name not in _STATE:
        _STATE[name] = R.loners() if name == "loners" else R.solve_scene(name)
    return _STATE[name]


@pytest.fixture
def exact(monkeypatch):
    monkeypatch.setenv("SPH_HIP_EXACT", "1")   # read by sph_create


def device_step(product_lib, st, P):
    mass, pos, vel, planes = st
    g = ffi.Context(product_lib, len(mass), planes)
    g.upload(mass, pos, vel)
    return g, g.step(P.to_ffi())


def assert_slot_order(g, where=""):
    """the device's own cell sort found nothing to do: host order IS slot order (uniform scenes)"""
    ci = g.download("cell_index").astype(np.int64)
    assert (np.diff(ci) >= 0).all(), where + "the upload order is not the device's slot order"


def fields_of(solver):
    return FIELDS if "density" in R.solves_of(solver) else STEP_FIELDS   # (OnlyDivergence writes no density_error)


def assert_stats_are_the_models(s, totals, where):
    where += "device %d %d %d %08x %08x, model %d %d %d %08x %08x" % (
        int(s.normal_count), int(s.negative_count), int(s.singular_count), bits(s.avg_error), bits(s.max_error),
        totals["normal"], totals["negative"], totals["singular"], bits(R.model_avg_error(totals)), bits(totals["max_err"]))
    assert (int(s.normal_count), int(s.negative_count), int(s.singular_count)) == (totals["normal"], totals["negative"], totals["singular"]), where
    assert bits(s.max_error) == bits(totals["max_err"]), where
    assert bits(s.avg_error) == bits(R.model_avg_error(totals)), where


# ---- (a) the sum, to the bit ----------------------------------------------------------------------------------------------------------
FORCED_CASES = [(s, sv, K) for s in R.SMALL for sv in ("IISPH", "OnlyDivergence", "HybridDFSPH") for K in R.FORCED_KS] + \
               [("trip-2", "IISPH", K) for K in R.FORCED_KS]   # (the large scene runs IISPH only: the 1026 partials are the same stage whatever the residual)


@pytest.mark.parametrize("scene,solver,K", FORCED_CASES, ids=lambda v: str(v))
def test_forced_solve_reports_the_models_sum(product_lib, oracle_lib, exact, scene, solver, K):
    st = state(scene)
    P = forced(max_iters=K, pressure_solver_method=solver)
    g, sg = device_step(product_lib, st, P)
    o, so = R.oracle_step(oracle_lib, st, P)
    where = f"{scene} {solver} K={K}: "
    assert sg.dt == so.dt, where
    assert_slot_order(g, where)
    assert_bit_identical(g, o, fields_of(solver), where)
    for which in R.solves_of(solver):
        s, t = R.stats_of(sg, which), R.stats_of(so, which)
        assert int(s.iters) == int(t.iters) == K, where
        _, totals = R.model_from_oracle(o, which)
        # (self-check: the model's counts are the oracle's own statistics)
        assert (totals["normal"], totals["negative"], totals["singular"]) == (int(t.normal_count), int(t.negative_count), int(t.singular_count)), where
        assert_stats_are_the_models(s, totals, where + which + ": ")
    g.close()
    o.close()


# ---- (b) the decision at its threshold -----------------------------------------------------------------------------------------------
def tolerances(solver, which, tol):
    """the solve under test at `tol`, the other solve of HybridDFSPH stopped at iteration 2 by HUGE_TOL (as in forced_tolerances)"""
    t = R.forced_tolerances(solver, which)
    t["div_tol" if which == "divergence" else "dens_tol"] = tol
    return t


def other_solve_stopped_at_2(solver, which, *stats):
    for w in R.solves_of(solver):
        if w != which:
            assert all(int(R.stats_of(s, w).iters) == 2 for s in stats)


@pytest.mark.parametrize("case", R.THRESHOLD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_the_solve_stops_exactly_where_the_models_value_passes(product_lib, oracle_lib, exact, case):
    scene, solver, which, K = case
    st = state(scene)
    rho0 = R.solve_params(solver, K).rest_density
    c = R.threshold_case(oracle_lib, st, solver, which, K, rho0)       # (asserts the bracket and that no iteration before K passes)
    where = f"{case}: tolerances {c['go']!r} / {c['stop']!r}: "
    # ON the bound (resp. the last tolerance whose threshold does not exceed the value): strict <, the solve goes on
    g, sg = device_step(product_lib, st, R.solve_params(solver, 50, **tolerances(solver, which, c["go"])))
    assert int(R.stats_of(sg, which).iters) > K, where + f"stopped at {int(R.stats_of(sg, which).iters)}"
    g.close()
    # the next float32 above: stops at K, and the step is the oracle's forced-K step
    g, sg = device_step(product_lib, st, R.solve_params(solver, 50, **tolerances(solver, which, c["stop"])))
    o, so = R.oracle_step(oracle_lib, st, R.solve_params(solver, K, **R.forced_tolerances(solver, which)))
    assert int(R.stats_of(sg, which).iters) == K == int(R.stats_of(so, which).iters), where + f"stopped at {int(R.stats_of(sg, which).iters)}"
    other_solve_stopped_at_2(solver, which, sg, so)
    assert sg.dt == so.dt
    assert_bit_identical(g, o, fields_of(solver), where)
    assert_stats_are_the_models(R.stats_of(sg, which), c["totals"], where)
    if K == 2 and scene != "trip-2":
        # max_iters beyond the progress word's 15 bits: the predicted queue instead of the paced solve -- the same decision, the same bits
        q, sq = device_step(product_lib, st, R.solve_params(solver, 32768, **tolerances(solver, which, c["stop"])))
        assert int(R.stats_of(sq, which).iters) == K, where
        other_solve_stopped_at_2(solver, which, sq)
        assert_bit_identical(q, g, fields_of(solver), where + "predicted queue: ")
        assert bits(R.stats_of(sq, which).avg_error) == bits(R.stats_of(sg, which).avg_error)
        q.close()
    g.close()
    o.close()


@pytest.mark.parametrize("solver", ["IISPH", "OnlyDivergence", "HybridDFSPH"])
def test_a_huge_tolerance_stops_at_iteration_two(product_lib, oracle_lib, exact, solver):
    """iter > 1: every residual passes 1e30 from iteration 0 on, the solve still runs iterations 0, 1 and 2 -- both residual modes"""
    st = state("blocks-7")
    g, sg = device_step(product_lib, st, R.solve_params(solver, 50, R.HUGE_TOL, R.HUGE_TOL))
    o, so = R.oracle_step(oracle_lib, st, R.solve_params(solver, 2))
    for which in R.solves_of(solver):
        assert int(R.stats_of(sg, which).iters) == 2 == int(R.stats_of(so, which).iters), which
    assert_bit_identical(g, o, fields_of(solver), solver + ": ")
    g.close()
    o.close()


@pytest.mark.parametrize("solver", ["IISPH", "OnlyDivergence", "HybridDFSPH"])
def test_all_particles_singular_stops_at_iteration_zero(product_lib, oracle_lib, exact, solver):
    """isolated particles, farther than a support from each other and the walls: a_ii = 0 everywhere, no "normal" particle -- the rule's
    first branch: iters == 0, a NaN average on both sides, zero pressures"""
    st = state("loners")
    P = R.solve_params(solver, 50, 1e-3, 1e-3)
    g, sg = device_step(product_lib, st, P)
    o, so = R.oracle_step(oracle_lib, st, P)
    for which in R.solves_of(solver):
        s, t = R.stats_of(sg, which), R.stats_of(so, which)
        assert int(s.iters) == 0 == int(t.iters), which
        assert (int(s.normal_count), int(s.negative_count), int(s.singular_count)) == (0, 0, len(st[0])) == (int(t.normal_count), int(t.negative_count), int(t.singular_count))
        assert np.isnan(s.avg_error) and np.isnan(t.avg_error)
    assert not g.download("pressure").any() and not o.download("pressure").any()
    assert_bit_identical(g, o, STEP_FIELDS, solver + ": ")
    g.close()
    o.close()


# ---- (c) the predicted free-running count --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FREE_CASES, ids=lambda c: c[0])
def test_free_running_count_is_the_models_prediction(product_lib, oracle_lib, exact, case):
    """Three consecutive steps (re-uploaded each step in the visiting order of the oracle's state, as stepwise does): K* = the first k >= 2
    at which the rule passes the MODEL's totals of the oracle forced to k; the margin to the threshold at K* and K* - 1 is a condition on
    the input (>= MARGIN_ULPS ulps of the compared value), asserted; the device's free-running solve stops at K* with the bits of the
    oracle's forced-K* step."""
    solver, which, tols, _ = case
    rho0 = R.solve_params(solver, 50).rest_density
    mass, pos, vel, planes = state("blocks-7")
    for step in range(R.FREE_STEPS):
        st = R.reordered(mass, pos, vel, planes)
        mass, pos, vel, planes = st
        k, margin, o, so = R.predicted_count(oracle_lib, st, solver, which, tols[step], rho0)
        where = f"{solver} step {step}: K* = {k}, margin {margin:.3g} ulps: "
        assert 4 <= k <= 10 and margin >= R.MARGIN_ULPS, where
        g, sg = device_step(product_lib, st, R.solve_params(solver, 50, **tolerances(solver, which, tols[step])))
        assert int(R.stats_of(sg, which).iters) == k, where + f"the device stopped at {int(R.stats_of(sg, which).iters)}"
        assert sg.dt == so.dt
        assert_slot_order(g, where)
        assert_bit_identical(g, o, fields_of(solver), where)
        _, totals = R.model_from_oracle(o, which)
        assert_stats_are_the_models(R.stats_of(sg, which), totals, where)
        pos, vel = o.download("position"), o.download("velocity")
        g.close()
        o.close()


# ---- (d) the same reduction behind the default policy's sweeps ------------------------------------------------------------------------
def two_sizes():
    """test_gpu_parity.test_adaptive_h_two_size_classes' construction (2:1 radius ratio, 828 + 207 = 1035 = 4 * 256 + 11 particles), the lattices drawn together by SQUEEZE, in
    the device's visiting order: the FINE particles' grid (device_order)"""
    scn = sc.SceneConfig(sc.SceneBoundary("box", 2.0, 2.0),
                         [sc.SceneFluidBlock([-0.95, -0.5], [0.55, 1.4], 0.03, 0.93, [0.5, 0]),
                          sc.SceneFluidBlock([-0.40, -0.5], [0.55, 1.4], 0.06, 0.93, [-0.5, 0])])
    pos, mass, vel = sc.init_particles(scn)
    corner = pos.min(axis=0)
    pos = (corner + (pos - corner) * F(R.SQUEEZE)).astype(F)   # (drawn together like the uniform scenes: at rest spacing 44 of the 1035 are "normal")
    perm = device_order(pos, h_from_mass(mass))
    return mass[perm], pos[perm], vel[perm], sc.boundary_planes(scn.boundary)


def model_from_device(g):
    """the model fed with what the DEVICE left: density_error, and the classes from a_ii and the final pressure (host order = slot order)"""
    err, aii, p = g.download("density_error"), g.download("aii"), g.download("pressure")
    cls = np.where(np.abs(aii) < F(10e-4), R.CLS_SINGULAR, np.where(p > 0, R.CLS_NORMAL, R.CLS_NEGATIVE)).astype(np.uint8)
    return R.device_residual_totals(err, cls)[1]


@pytest.mark.parametrize("scene", R.SMALL + ("trip-2", "two-sizes"))
def test_default_policy_reduces_in_the_same_order(product_lib, monkeypatch, scene):
    """FAST policy, IISPH (density residual): a uniform scene runs sweep B as OpJacobiU on records and offset lists, the two-size scene as
    the generic OpJacobi on mask and index lists -- each with its own call of the epilogue.  Forced K = 3: counts and the bits of avg_error
    and max_error are the model's of the device's own residuals; then the threshold pair around the model's value of forced K = 2: the
    decision on the path the benchmark runs."""
    monkeypatch.delenv("SPH_HIP_EXACT", raising=False)
    uniform = scene != "two-sizes"
    st = state(scene) if uniform else two_sizes()
    assert (np.ptp(st[0]) == 0) == uniform
    g, sg = device_step(product_lib, st, forced(max_iters=3, pressure_solver_method="IISPH"))
    assert g.math_policy() == "fast"
    if uniform:
        assert_slot_order(g, scene + ": ")   # (two sizes: cell_index is the reference's coarse grid; the slot order is device_order's fine grid)
    assert int(sg.density_solver.iters) == 3
    totals = model_from_device(g)
    assert totals["normal"] > 0.3 * len(st[0]), "the scene has too few normal particles for the sum to say anything"
    assert_stats_are_the_models(sg.density_solver, totals, f"{scene} K=3: ")
    g.close()
    # the threshold pair around the model's value of the device's forced K = 2
    g, sg = device_step(product_lib, st, forced(max_iters=2, pressure_solver_method="IISPH"))
    totals = model_from_device(g)
    assert_stats_are_the_models(sg.density_solver, totals, f"{scene} K=2: ")
    ref = {f: g.download(f) for f in FIELDS}
    g.close()
    rho0 = dam_break_params().rest_density
    go, stop = R.bracketing_tolerances(totals, 1, rho0, float(sg.dt))
    g, s1 = device_step(product_lib, st, R.solve_params("IISPH", 50, dens_tol=go))
    assert int(s1.density_solver.iters) > 2, (scene, go)
    g.close()
    g, s2 = device_step(product_lib, st, R.solve_params("IISPH", 50, dens_tol=stop))
    assert int(s2.density_solver.iters) == 2, (scene, stop)
    for f in FIELDS:      # ... and the step is the forced-2 step of the same policy
        assert np.array_equal(g.download(f), ref[f]), (scene, f)
    g.close()


# ---- (e) slab groups --------------------------------------------------------------------------------------------------------------------
def slab_cuts(pos, ranks):
    """two ranks: the column halved; three: the same two and a third that owns nothing and is no neighbour of a ghost"""
    x_hi = float(pos[:, 0].max())
    return [-D.INF, float(np.median(pos[:, 0]))] + ([x_hi + 0.15] if ranks == 3 else []) + [D.INF]


class _Group:
    def __init__(self, lib, st, transport, ranks):
        mass, pos, vel, planes = st
        cuts = slab_cuts(pos, ranks)
        self.thr = D.ThreadedGroup(lib, pos, mass, vel, planes, ranks, cuts=cuts) if transport == "threads" else None
        self.contexts = self.thr.contexts if self.thr else D.make_loopback_group(lib, pos, mass, vel, planes, ranks, cuts=cuts)

    def step(self, p):
        return self.thr.step(p) if self.thr else ffi.group_step(self.contexts, p)

    def close(self):
        if self.thr:
            self.thr.close()
        else:
            for c in self.contexts:
                c.close()


@pytest.mark.parametrize("transport,ranks,K,split", [("loopback", 2, 2, False), ("loopback", 2, 3, True), ("loopback", 3, 2, True), ("loopback", 3, 3, False),
                                                     ("threads", 3, 2, True)])
@pytest.mark.parametrize("solver,which", [("IISPH", "density"), ("OnlyDivergence", "divergence")])
def test_slab_ranks_decide_together(product_lib, monkeypatch, transport, ranks, K, split, solver, which):
    """Groups of two and of three slabs on the 1600-particle scene, forced K = 2 and 3 in each; of three ranks the third is an EMPTY slab
    (its decisions come from launch_solver_progress).  split: sweep A in
    two launches -- interior beside the exchange, k_solver_progress decides between them, then the edge (DECIDE_NOT_HERE).  The condition
    (sph_step.hip: split_sweep_a) is SPH_OVERLAP = 1, or by default a rank of at least SPLIT_MIN_PARTICLES = 786 432 particles, which is
    not test-sized: the tests' switch is used, and that the split form really ran is read from the profile (SphDistStats does not show
    it).  Forced K: every rank reports K and the same bits of avg_error; K = 2: the threshold pair around the GROUP's own value flips the
    count on all ranks together."""
    monkeypatch.delenv("SPH_HIP_EXACT", raising=False)
    monkeypatch.setenv("SPH_OVERLAP", "1" if split else "0")
    st = state("blocks-7")
    rho0 = dam_break_params().rest_density

    def run(P, profile=False):
        grp = _Group(product_lib, st, transport, ranks)
        try:
            assert [c.n for c in grp.contexts][2:] == [0] * (ranks - 2) and all(c.n > 256 for c in grp.contexts[:2])
            if profile:
                grp.contexts[1].profile_enable(1)
            stats = grp.step(P.to_ffi())
            if profile:
                prof = grp.contexts[1].profile_get()
                assert ("pressure_accel_edge" in prof) == split and ("solver_progress" in prof) == split
            return [(float(s.dt), int(R.stats_of(s, which).iters), bits(R.stats_of(s, which).avg_error), int(R.stats_of(s, which).normal_count)) for s in stats]
        finally:
            grp.close()

    at_k = run(R.solve_params(solver, K), profile=True)
    assert len(set(at_k)) == 1 and at_k[0][1] == K and at_k[0][3] > 0, at_k
    if K != 2:
        return
    dt, _, avg_bits, _ = at_k[0]
    go, stop = R.bracket_average(np.array([avg_bits], np.uint32).view(F)[0], R.residual_mode(which), rho0, dt)   # (the group's OWN average)
    on = run(R.solve_params(solver, 50, **tolerances(solver, which, go)))
    assert len(set(on)) == 1 and on[0][1] > 2, on
    above = run(R.solve_params(solver, 50, **tolerances(solver, which, stop)))
    assert len(set(above)) == 1 and above[0][1] == 2 and above[0][2] == avg_bits, above
