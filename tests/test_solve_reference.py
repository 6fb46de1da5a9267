"""tests/solve_reference.py -- the device's residual reduction restated in numpy float32 -- against itself, and the constructions
tests/test_gpu_solve_decision.py rests on, checked where no GPU is needed (CPU oracle only):

  * the model on integer-valued residuals (every partial sum exact) is the exact sum at every size at which a stage takes another
    path; max_err and the counts are numpy's; idle (class 3) lanes change nothing;
  * the ORDER is visible in the bits on the inputs the GPU tests use: the model's sum_err of the oracle's residuals differs from a
    sequential sum, from the oracle's own (chunks of 1024) and from the model with one stage in another order -- per stage on the scenes
    recorded in ORDER_WITNESSES.  A scene on which the other order gives the same bits pins nothing for that stage, so the witnesses
    were chosen from a scan over (scene, solver, K in FORCED_KS); stage 3's only witness is the 1026-partial scene (a thread needs
    three partials for its chain to have an order).  Rows or lanes REVERSED cannot be a witness of stage 1: see solve_reference.py.
  * the threshold constructions: the two tolerances of every case of THRESHOLD_CASES are adjacent float32 values whose thresholds, formed
    as solver_stop_rule forms them, bracket the model's value -- so the GPU test cannot pass vacuously; the free-running cases have
    K* in 4 .. 10 with the margin asserted, over the three steps.
"""
import numpy as np
import pytest

from tests import solve_reference as R
from tests.oracle_harness import load_oracle

F = np.float32
SIZES = [1, 63, 64, 65, 255, 256, 257, 1599, 1600, 262656]


def bits(x):
    return int(np.asarray(x, F).view(np.uint32))


@pytest.fixture(scope="module")
def oracle():
    return load_oracle()


def integer_case(n, seed=0):
    rng = np.random.default_rng(seed + n)
    err = rng.integers(-30, 31, n).astype(F)           # |any partial sum| <= 30 * 262 656 < 2^24: exact in float32 in ANY order
    cls = rng.choice([0, 0, 0, 1, 2], n).astype(np.uint8)
    return err, cls


@pytest.mark.parametrize("n", SIZES)
def test_integer_residuals_give_the_exact_sum_and_numpys_counts(n):
    err, cls = integer_case(n)
    partials, t = R.device_residual_totals(err, cls)
    normal = cls == 0
    assert float(t["sum_err"]) == float(err[normal].astype(np.int64).sum())
    assert float(t["max_err"]) == float(np.abs(err[normal]).max(initial=0.0))
    assert (t["normal"], t["singular"], t["negative"]) == tuple(int(np.count_nonzero(cls == k)) for k in (0, 1, 2))
    nb = (n + 255) // 256
    assert all(len(partials[k]) == nb for k in partials)
    pad = np.zeros(nb * 256, np.int64)
    pad[:n] = np.where(normal, err, 0)
    assert np.array_equal(partials["sum_err"].astype(np.int64), pad.reshape(nb, 256).sum(axis=1))
    for order in R.ORDERS[1:]:     # ... and exact sums do not see the order
        assert bits(R.device_residual_totals(err, cls, order)[1]["sum_err"]) == bits(t["sum_err"])


@pytest.mark.parametrize("n", [1, 63, 255, 256, 1599])
@pytest.mark.parametrize("idle", [1, 64, 300])
def test_idle_lanes_change_nothing(n, idle):
    err, cls = integer_case(n, 7)
    err = (err * F(0.37)).astype(F)                     # (inexact sums: an idle lane that entered would be seen)
    _, t = R.device_residual_totals(err, cls)
    err2 = np.concatenate([err, np.full(idle, 1e6, F)])
    cls2 = np.concatenate([cls, np.full(idle, R.CLS_IDLE, np.uint8)])
    p2, t2 = R.device_residual_totals(err2, cls2)
    assert {k: bits(v) if k.endswith("err") else v for k, v in t.items()} == {k: bits(v) if k.endswith("err") else v for k, v in t2.items()}


def test_a_mirrored_balanced_tree_is_the_same_tree():
    """why stage 1's other order is a rotation: lanes reversed inside every wave give the same bits on random floats"""
    rng = np.random.default_rng(1)
    err = rng.normal(0, 1, 64 * 40).astype(F)
    cls = np.zeros(len(err), np.uint8)
    a, _ = R.device_residual_totals(err, cls)
    b, _ = R.device_residual_totals(err.reshape(-1, 64)[:, ::-1].reshape(-1), cls)
    assert np.array_equal(a["sum_err"].view(np.uint32), b["sum_err"].view(np.uint32))
    c, _ = R.device_residual_totals(err, cls, "rows-rotated")
    assert not np.array_equal(a["sum_err"].view(np.uint32), c["sum_err"].view(np.uint32))


_RESIDUALS = {}


def residuals(oracle, scene, solver, which, K):
    """the oracle's per-particle residuals and classes of iteration K, computed once per case"""
    key = (scene, solver, which, K)
    if key not in _RESIDUALS:
        o, so = R.oracle_step(oracle, R.solve_scene(scene), R.solve_params(solver, K, **R.forced_tolerances(solver, which)))
        res, cls = o.solve_residuals(which)
        s = R.stats_of(so, which)
        _RESIDUALS[key] = (res, cls, F(s.avg_error), int(s.normal_count))
        o.close()
    return _RESIDUALS[key]


def sequential_sum(v):
    return np.add.accumulate(np.asarray(v, F), dtype=F)[-1]      # (accumulate IS one-at-a-time; a pairwise library sum is not used)


def oracle_sum(res, cls):
    """oracle/step.c single_pressure_iteration: chunks of 1024 particles summed one at a time, the chunk sums added in index order"""
    v = np.where(cls == 0, res, F(0)).astype(F)
    return sequential_sum([sequential_sum(np.concatenate([[F(0)], v[b:b + 1024][cls[b:b + 1024] == 0]])) for b in range(0, len(v), 1024)])


# stage -> the (scene, solver, solve, K) on which that stage's other order changes the bits of the TOTAL (from the scan; K of FORCED_KS)
ORDER_WITNESSES = {
    "rows-rotated": [("one-wave", "IISPH", "density", 2), ("blocks-7", "IISPH", "density", 5)],
    "waves-reversed": [("tail-63", "IISPH", "density", 2), ("blocks-7", "OnlyDivergence", "divergence", 5)],
    "partials-reversed": [("trip-2", "IISPH", "density", 2)],
}


@pytest.mark.parametrize("order", list(ORDER_WITNESSES))
def test_each_stages_order_is_visible_on_the_gpu_tests_inputs(oracle, order):
    for case in ORDER_WITNESSES[order]:
        res, cls, avg, normal = residuals(oracle, *case)
        _, t = R.device_residual_totals(res, cls)
        _, u = R.device_residual_totals(res, cls, order)
        assert (t["normal"], u["normal"]) == (normal, normal)
        assert bits(t["sum_err"]) != bits(u["sum_err"]), (order, case)


def scanned_cases(scene):
    """every (scene, solver, solve, K) the GPU tests force on `scene`"""
    return [(scene, sv, w, K) for sv, w in (R.SOLVES if scene != "trip-2" else R.SOLVES[:1]) for K in R.FORCED_KS]


# The scan over scanned_cases of every scene found these cases on which the model's sum ROUNDS ALIKE with the oracle's chunk sum / the
# sequential sum (bits equal; recorded so that the choice of witnesses can be reproduced; not asserted -- that two orders agree somewhere
# is chance, not a property):
#   both:        one-wave IISPH 0, OnlyDivergence 0, HybridDFSPH divergence 0, HybridDFSPH density 2 (at most 56 addends);
#                tail-63 OnlyDivergence 5, HybridDFSPH divergence 5, HybridDFSPH density 0
#   the oracle:  blocks-7 IISPH 1 and 5; trip-2 IISPH 2        sequential:  blocks-7 IISPH 2; xcd-2 IISPH 0
# Every other case differs from both; asserted per scene: at least three quarters of its cases differ from each.
@pytest.mark.parametrize("scene", list(R.SCENES))
def test_the_models_sum_is_neither_sequential_nor_the_oracles(oracle, scene):
    cases = scanned_cases(scene)
    differs_from_oracle, differs_from_sequential = [], []
    for case in cases:
        res, cls, avg, normal = residuals(oracle, *case)
        _, t = R.device_residual_totals(res, cls)
        own = oracle_sum(res, cls)
        assert bits(own / F(normal)) == bits(avg), "the restated chunk sum is not the oracle's own"
        assert abs(float(t["sum_err"]) - float(own)) <= 1e-5 * abs(float(own))     # (the same addends all the same)
        if bits(t["sum_err"]) != bits(own):
            differs_from_oracle.append(case)
        if bits(t["sum_err"]) != bits(sequential_sum(res[cls == 0])):
            differs_from_sequential.append(case)
    assert 4 * len(differs_from_oracle) >= 3 * len(cases), differs_from_oracle
    assert 4 * len(differs_from_sequential) >= 3 * len(cases), differs_from_sequential


@pytest.mark.parametrize("case", R.THRESHOLD_CASES, ids=lambda c: "-".join(map(str, c)))
def test_threshold_tolerances_are_adjacent_and_bracket_the_models_value(oracle, case):
    scene, solver, which, K = case
    rho0 = R.solve_params(solver, K).rest_density
    c = R.threshold_case(oracle, R.solve_scene(scene), solver, which, K, rho0)
    go, stop = F(c["go"]), F(c["stop"])
    assert np.nextafter(go, F(np.inf)) == stop and float(go) == c["go"] and float(stop) == c["stop"]
    lhs, thr = R.stop_measure(c["totals"], R.residual_mode(which), rho0, c["dt"])
    assert thr(go) <= lhs < thr(stop)
    if which == "density":
        assert go == lhs, "density mode: the looser tolerance is ON the bound"
    rule = dict(residual_density=R.residual_mode(which), max_iters=50)
    assert not R.predicted_stop(c["totals"], K, dict(rule, max_avg_error=c["go"]), rho0, c["dt"])
    assert R.predicted_stop(c["totals"], K, dict(rule, max_avg_error=c["stop"]), rho0, c["dt"])
    assert not R.predicted_stop(c["totals"], 1, dict(rule, max_avg_error=R.HUGE_TOL), rho0, c["dt"])      # (iter > 1)


@pytest.mark.parametrize("case", R.FREE_CASES, ids=lambda c: c[0])
def test_free_running_tolerances_give_a_count_in_range_with_margin(oracle, case):
    solver, which, tols, recorded = case
    rho0 = R.solve_params(solver, 50).rest_density
    mass, pos, vel, planes = R.solve_scene("blocks-7")
    counts = []
    for step in range(R.FREE_STEPS):
        state = R.reordered(mass, pos, vel, planes)
        mass, pos, vel, planes = state
        k, margin, o, so = R.predicted_count(oracle, state, solver, which, tols[step], rho0)
        assert 4 <= k <= 10 and margin >= R.MARGIN_ULPS, (step, k, margin)
        counts.append(k)
        pos, vel = o.download("position"), o.download("velocity")
        o.close()
    assert tuple(counts) == recorded      # (how the tolerances were picked)
