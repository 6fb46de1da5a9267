"""What the scenes of tests/branch_point_scenes.py hold, proved on the CPU: every branch population counted with the kernels' own f32
expressions, the oracle inside its bars against the dense f64 restatement on every scene (tests/test_oracle_independent.py: `_compare`
at tol = 1), the oracle's neighbour sets equal to the numpy f32 predicate entry by entry, and the penalty kinds distinguishable.
tests/test_gpu_branch_points.py runs the same scenes on the device."""
import numpy as np
import pytest

from adaptive_sph_amd import ffi
from tests import branch_point_scenes as B
from tests.neighbour_scenes import csr_keys, h_of_mass
from tests.oracle_harness import load_oracle
from tests.test_oracle_independent import _compare, compare_level_on


def oracle_step(s, P, steps=1):
    o = ffi.Context(load_oracle(), len(s["mass"]), s["planes"])
    o.upload(s["mass"], s["pos"], s["vel"])
    for _ in range(steps):
        o.step(P.to_ffi())
    return o


def keys_of_sets(nb):
    i, j = np.nonzero(nb)
    return (i.astype(np.uint64) << np.uint64(32)) | j.astype(np.uint64)


def oracle_sets_equal_f32_predicate(s, k_ext=None):
    """the step's lists (k = 2) and, built for the same positions, the extended lists of range `k_ext`"""
    o = oracle_step(s, B.case_params(0))
    assert np.array_equal(csr_keys(*o.download_neighbors()), keys_of_sets(B.f32_neighbour_sets(s["pos"], s["mass"], 2.0)))
    if k_ext is not None:
        o.upload_field("position", s["pos"])          # (the step moved them; h2 stays)
        assert load_oracle().lib.oracle_build_neighbors(o.handle, float(k_ext)) == 0
        assert np.array_equal(csr_keys(*o.download_neighbors()), keys_of_sets(B.f32_neighbour_sets(s["pos"], s["mass"], k_ext)))
    o.close()


# ---- wall distances -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_sizes", [False, True])
@pytest.mark.parametrize("handler", ["AnalyticOverestimate", "AnalyticUnderestimate"])
def test_wall_depths_holds_every_interval_and_every_branch_value(handler, two_sizes):
    s = B.wall_depths(handler, two_sizes)
    assert len(s["mass"]) <= 1500
    pop = B.wall_populations(s)
    assert min(pop["deep"], pop["behind"], pop["front"]) >= 20, pop
    assert pop["corner"] >= 3 and pop["floor_behind"] >= 20 and pop["floor_min"] < -0.6, pop
    d = pop["hand"]
    assert d["-1"] == -1.0 and d["-0.5"] == -0.5 and d["0"] == 0.0 and d["1"] == 1.0
    for name in ("-1", "-0.5", "0", "1"):        # the representable x on either side: the nearest d this particle size can have there
        assert d[name + "-"] < d[name] and abs(float(d[name + "-"]) - float(d[name])) < 4e-6
        if name != "1":
            assert d[name + "+"] > d[name] and abs(float(d[name + "+"]) - float(d[name])) < 4e-6
    assert d["1-"] < 1.0 and d["0+"] > 0.0 and d["0-"] < 0.0
    # only the left wall reaches the hand-placed particles (the polygon's nearest edge there is that wall: the same d)
    h = h_of_mass(s["mass"])
    hand = np.array(list(s["hand"].values()))
    for plane in s["box"][1:]:
        assert (B.wall_d(s["pos"][hand], h[hand], plane) >= 1.0).all()


@pytest.mark.parametrize("handler", ["AnalyticOverestimate", "AnalyticUnderestimate"])
def test_penalty_terms_are_distinguishable_on_wall_depths(handler):
    """lambda_sum = sum lambda(d) penalty(d) after one oracle step: the four terms differ pairwise, and exactly where their definitions
    do -- Quadratic1 from None at d < 0, Quadratic2 from Quadratic1 at d < 0 as well, Linear everywhere."""
    s = B.wall_depths(handler)
    lam = {}
    for pen in B.PENALTIES:
        o = oracle_step(s, B.case_params(0, boundary_penalty_term=pen, init_boundary_handler=handler))
        lam[pen] = o.download("lambda_sum")
        o.close()
    for a in range(4):
        for b in range(a + 1, 4):
            assert (lam[B.PENALTIES[a]] != lam[B.PENALTIES[b]]).sum() >= 20, (B.PENALTIES[a], B.PENALTIES[b])
    hand = s["hand"]
    for name in ("0", "0+", "1-"):               # in front of and on the wall the three non-linear terms are 1
        assert lam["None"][hand[name]] == lam["Quadratic1"][hand[name]] == lam["Quadratic2"][hand[name]] > 0
    assert lam["None"][hand["1"]] == 0 and lam["None"][hand["1-"]] > 0            # d < 1 decides whether there is a term at all
    # lambda is the constant 1 from d = -1 down, read from the table above it: the penalty alone differs at the knees
    assert lam["None"][hand["-1"]] == 1.0 == lam["None"][hand["-1-"]] and lam["None"][hand["-1+"]] <= 1.0
    assert lam["Quadratic1"][hand["-1"]] == 1.5 and lam["Quadratic2"][hand["-1"]] == 1.75
    # Quadratic2's knee: 0.75 - d at d <= -0.5, d d + 1 above it (both 1.25 at the knee itself: the side shows one step beside it)
    lm = lam["None"]
    for name in ("-0.5-", "-0.5", "-0.5+"):
        d = np.float32(B.wall_populations(s)["hand"][name])
        want = np.float32(0.75) - d if d <= -0.5 else d * d + np.float32(1.0)
        assert lam["Quadratic2"][hand[name]] == lm[hand[name]] * want, name
    if handler == "AnalyticOverestimate":
        return
    planes = B.wall_depths("AnalyticOverestimate")
    o = oracle_step(planes, B.case_params(0, boundary_penalty_term="Quadratic2"))
    idx = np.array(list(hand.values()))
    assert np.array_equal(o.download("lambda_sum")[idx], lam["Quadratic2"][idx])
    o.close()


WALL_CASES = [("HybridDFSPH", 3, pen, False) for pen in B.PENALTIES] + [("IISPH", 0, "Quadratic1", False), ("IISPH", 3, "Quadratic2", False),
                                                                         ("HybridDFSPH", 0, "Quadratic1", False), ("HybridDFSPH", 3, "Quadratic2", True)]


@pytest.mark.parametrize("solver,max_iters,pen,two_sizes", WALL_CASES)
def test_oracle_against_dense_f64_on_wall_depths(solver, max_iters, pen, two_sizes):
    s = B.wall_depths(two_sizes=two_sizes)
    o = ffi.Context(load_oracle(), len(s["mass"]), s["planes"])
    _compare(o, s["pos"], s["mass"], s["vel"], B.case_params(max_iters, solver, boundary_penalty_term=pen), max_iters, 1.0, s["box"], block=False)
    o.close()


# ---- close pairs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_sizes", [False, True])
def test_close_pairs_holds_its_groups(two_sizes):
    s = B.close_pairs(two_sizes)
    assert len(s["mass"]) <= 1500
    i, j = np.array([p[0] for p in s["pairs"]]), np.array([p[1] for p in s["pairs"]])
    group = np.array([p[2] for p in s["pairs"]])
    q = B.pair_q(s["pos"], s["mass"], i, j)
    exact = (s["pos"][i] == s["pos"][j]).all(axis=1)
    assert exact.sum() == 16 and (q[exact] == 0).all() and (group[exact] == "zero").all()
    assert ((q > 0) & (q < B.Q_FAST_ZERO)).sum() >= 12
    band = (q >= 1e-7) & (q <= B.Q_CUTOFF)
    assert band.sum() >= 12 and (np.abs(q - 5e-6) < 3e-7).sum() >= 3 and (np.abs(q - 9e-6) < 3e-7).sum() >= 3
    assert ((q > B.Q_CUTOFF) & (q <= 1.2e-5)).sum() >= 12 and (np.abs(q - 1e-3) < 2e-4).sum() >= 12
    # (the cut-off is an f32 comparison in the reference: nobody stands within rounding of it)
    assert (np.abs(q - B.Q_CUTOFF) > 1e-7).all()
    hosts, counts = np.unique(i, return_counts=True)
    assert (counts == 2).sum() == 2 and (counts <= 2).all()                          # two triples at one point
    assert (np.abs(s["vel"][i] - s["vel"][j]).max(axis=1) > 0).all()                 # a partner does not move with its host
    if two_sizes:
        assert (s["mass"][i] != s["mass"][j]).sum() >= 12
    cq = B.close_partners(s)
    assert np.isfinite(cq).sum() == len(s["pairs"]) + len(hosts)


CLOSE_CASES = [("IISPH", 0, False), ("IISPH", 3, False), ("HybridDFSPH", 0, False), ("HybridDFSPH", 3, False), ("HybridDFSPH", 3, True), ("IISPH", 0, True)]


@pytest.mark.parametrize("solver,max_iters,two_sizes", CLOSE_CASES)
def test_oracle_against_dense_f64_on_close_pairs(solver, max_iters, two_sizes):
    s = B.close_pairs(two_sizes)
    o = ffi.Context(load_oracle(), len(s["mass"]), s["planes"])
    _compare(o, s["pos"], s["mass"], s["vel"], B.case_params(max_iters, solver), max_iters, 1.0, (), block=False)
    o.close()


# ---- the edge of the support ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_sizes", [False, True])
@pytest.mark.parametrize("k", [2.0, "extended"])
def test_support_edge_pairs_stand_where_they_should(k, two_sizes):
    k = B.k_extended() if k == "extended" else np.float32(k)
    s = B.support_edge(k, two_sizes, clumps=k != 2.0)
    assert (np.abs(s["pos"][[p[0] for p in s["pairs"]]]) < 0.02).all()
    nb = B.f32_neighbour_sets(s["pos"], s["mass"], k)
    seen = {kind: 0 for kind in B.EDGE_KINDS}
    both_forms = 0
    for i, j, kind in s["pairs"]:
        r2, s2 = B.predicate_terms(s["pos"], s["mass"], i, j, k)
        assert B.predicate_terms(s["pos"], s["mass"], j, i, k) == (r2, s2)           # the pair reads the same from either side
        if kind == "equal":
            assert r2 == s2 and not nb[i, j]
        elif kind == "below":
            assert r2 == B.below(s2) and nb[i, j]
        elif kind == "above":
            assert r2 == B.above(s2) and not nb[i, j]
        else:
            dx, dy = s["pos"][i] - s["pos"][j]
            ca, cb = B.contracted_r2(dx, dy)
            assert (ca < s2) != (r2 < s2)
            both_forms += int((cb < s2) != (r2 < s2))
        seen[kind] += 1
    assert min(seen["equal"], seen["below"], seen["above"]) >= 4 and seen["contracted"] >= 8, seen
    assert both_forms >= 4, both_forms
    if two_sizes:
        assert sum(s["mass"][i] != s["mass"][j] for i, j, _ in s["pairs"]) >= 8
    for a, b, c, kind in s["clumps"]:
        assert nb[a].sum() == (3 if kind == "below" else 2) and nb[a, c] and nb[a, b] == (kind == "below")
    oracle_sets_equal_f32_predicate(s, k)


@pytest.mark.parametrize("two_sizes", [False, True])
def test_oracle_against_dense_f64_on_support_edge(two_sizes):
    """(the neighbour relation from the f32 predicate: f64 places the edge pairs on either side, and only the count tells)"""
    s = B.support_edge(2.0, two_sizes)
    o = ffi.Context(load_oracle(), len(s["mass"]), s["planes"])
    _compare(o, s["pos"], s["mass"], s["vel"], B.case_params(3), 3, 1.0, (), block=False, nb=B.f32_neighbour_sets(s["pos"], s["mass"], 2.0))
    o.close()


@pytest.mark.parametrize("two_sizes", [False, True])
def test_the_insufficient_neighbours_flag_is_the_edge_predicate_of_the_extended_lists(two_sizes):
    """the host of a clump has two or three entries on its extended list with the pair on the edge: `fewer than 3 entries` tells which"""
    s = B.support_edge(B.k_extended(), two_sizes, clumps=True)
    o = oracle_step(s, B.case_params(2, level_estimation_method="EmptyAngle", maximum_surface_distance=0.2))
    flag = o.download("flag_insufficient_neighs").astype(bool)
    o.close()
    assert [bool(flag[a]) for a, _, _, _ in s["clumps"]] == [kind != "below" for _, _, _, kind in s["clumps"]]


@pytest.mark.parametrize("scene", ["wall_depths", "wall_depths_two_sizes", "close_pairs", "close_pairs_two_sizes", "wall_records"])
def test_oracle_sets_equal_the_f32_predicate(scene):
    s = {"wall_depths": B.wall_depths, "wall_depths_two_sizes": lambda: B.wall_depths(two_sizes=True), "close_pairs": B.close_pairs,
         "close_pairs_two_sizes": lambda: B.close_pairs(True), "wall_records": B.wall_records}[scene]()
    oracle_sets_equal_f32_predicate(s, B.k_extended())


# ---- level estimation, and the scene of the record forms -------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["close_pairs", "close_pairs_two_sizes", "wall_depths"])
def test_oracle_level_estimation_against_dense_restatement_on_branch_scenes(scene):
    """the detector's |x_j - x_i| + 1e-6 over pairs at r = 0 and r ~ 1e-9, the normal with the gradient's cut-off, and the rule that a
    particle closer than 1.5 h to a wall -- behind it included -- is interior"""
    s = {"close_pairs": B.close_pairs, "close_pairs_two_sizes": lambda: B.close_pairs(True), "wall_depths": B.wall_depths}[scene]()
    P = B.case_params(2, level_estimation_method="EmptyAngle", maximum_surface_distance=0.2)
    o = ffi.Context(load_oracle(), len(s["mass"]), s["planes"])
    compare_level_on(o, s["pos"], s["mass"], s["vel"], P, s["planes"], "SurfaceDistanceMiddle", 1.0, scene == "wall_depths", block=False)
    o.close()


def test_wall_records_runs_its_steps_and_holds_what_the_forms_need():
    s = B.wall_records()
    h = h_of_mass(s["mass"])
    assert np.ptp(h) == 0 and 20 <= (B.wall_d(s["pos"], h, B.LEFT) <= 0).sum() < len(h) // 10
    o = ffi.Context(load_oracle(), len(s["mass"]), s["planes"])
    o.upload(s["mass"], s["pos"], s["vel"])
    p = B.wall_records_params().to_ffi()
    longest = []
    for _ in range(B.RECORD_STEPS):
        o.step(p)                                     # (raises on any error of the step)
        off, _ = o.download_neighbors()
        longest.append(int(np.diff(off.astype(np.int64)).max()) - 1)
        assert (o.download("lambda_sum") != 0).sum() >= 20 and np.isfinite(o.download("position")).all()
    assert longest[0] > B.NLOFF_SLOTS and longest[1] > B.NLOFF_SLOTS, longest     # in the first step and in one that starts from a merge
    o.close()
