"""The device's wall loads (include/sph_wall_load.h) against their restatement in numpy and Python ints (tests/wall_load_reference.py), byte
for byte: every comparison feeds the twin with the context's own downloaded m, x, h, rho, p (a plain context downloads in reference
order: the id is the index) and compares the whole sph_wall_load_result and the profile's words.  The twin itself is tied to the step by
tests/test_wall_load_host.py."""
import csv
import io
from pathlib import Path

import numpy as np
import pytest

from adaptive_sph_amd import distributed as D, ffi, scene as sc, wall_loads
from adaptive_sph_amd.workloads import dam_break_params
from tests import ledger_reference as lr, wall_load_reference as wr, wall_load_scenes as ws

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
EVERY = ["mass", "position", "velocity", "density", "aii", "constant_field", "ppe_source_term", "pressure", "pressure_accel", "level_estimation", "stash",
         "neighbor_count", "particle_size_class", "flag_is_fluid_surface", "flag_insufficient_neighs", "flag_neighborhood_reduced", "h2",
         "cell_index", "h2_next", "level_old", "lambda_sum", "lambda_grad_sum"]
f32 = np.float32
BOX = sc.SceneBoundary("box", 4.0, 2.0)
PLANES = sc.boundary_planes(BOX)                     # left, right, floor, ceiling
POLYGON = sc.boundary_planes(BOX, "AnalyticUnderestimate")
LEFT, RIGHT, FLOOR, CEILING = range(4)
FLOOR_RANGE = (-2.0, 2.0)                            # the floor's s = -x over the box; 4 / B and B / 4 are exact for B = 1, 7, 4096


def _state(ctx, p, ids=None):
    return lr.Particles({f: ctx.download(f) for f in ws.FIELDS}, ids, float(p.rest_density))


def _same(ctx, p, boundary, bins=0, ranges=None, exps=None, label=""):
    """the device's result and profile words equal the twin's, byte for byte -> (device, twin result, twin profile, twin wall)"""
    wall = wr.Wall.of(boundary, ws.luts(), p)
    kind, want, prof = wr.wall_load(_state(ctx, p), wall, bins, ranges, exps)
    assert kind == "ok", want
    got = wall_loads.wall_load(ctx, p, bins, ranges, exps)
    assert bytes(got) == wr.result_bytes(want), (label, got.raw, [e["raw"] for e in want["elements"]], got.exponents, [e["exponent"] for e in want["elements"]],
                                                 got.n_entries, [e["n_entries"] for e in want["elements"]], got.n_unbinned)
    if bins:
        assert got.words.tobytes() == wr.profile_bytes(prof, wall.n_elements, bins), label
    else:
        assert got.words is None
    return got, want, prof, wall


def _refused(ctx, p, boundary, text=None, status=1, **kw):
    """the twin refuses with a sentence and the device with the same one (text: the device's alone, for what the twin is not asked)"""
    if text is None:
        kind, text, _ = wr.wall_load(_state(ctx, p), wr.Wall.of(boundary, ws.luts(), p), kw.get("bins", 0), kw.get("ranges"), kw.get("exps"))
        assert kind == "refused", text
    with pytest.raises(ffi.SphError) as e:
        wall_loads.wall_load(ctx, p, kw.get("bins", 0), kw.get("ranges"), kw.get("exps"))
    assert e.value.status == status and text in str(e.value), (text, str(e.value))
    return text


def _stepped(product_lib, pos, mass, vel, boundary, P, steps, policy="fast"):
    ctx = ffi.Context(product_lib, len(mass) + 8, boundary)
    if policy != "fast":
        ctx.set_math_policy(policy)
    ctx.upload(mass, pos, vel)
    p = P.to_ffi()
    for _ in range(steps):
        ctx.step(p)
    return ctx, p


# ---- 1. the corners scene: policies, the polygon, the symmetric gradient, every penalty term -----------------------------------------
CASES = [("AnalyticOverestimate", pen, "ConsistentSimpleGradient", "fast") for pen in ws.PENALTIES] + [
    ("AnalyticOverestimate", "Quadratic1", "ConsistentSimpleGradient", "exact"),
    ("AnalyticOverestimate", "Quadratic1", "ConsistentSymmetricGradient", "fast"),
    ("AnalyticUnderestimate", "Quadratic1", "ConsistentSimpleGradient", "fast")]


@pytest.mark.parametrize("handler,pen,op,policy", CASES)
def test_corners_scene(product_lib, handler, pen, op, policy):
    """corners_scene with five isolated strays at and beyond the walls, two steps (one under the symmetric gradient): particles with two entries (the corners), d on every
    branch of the penalty terms, lambda = 1 beyond d = -1."""
    scn, pos, mass, vel, strays = ws.strays_scene()
    boundary = sc.boundary_planes(scn.boundary, handler)
    # (under the symmetric gradient the squeezed lattice's second step ends in SPH_ERR_AII_NEGATIVE: one step there)
    steps = 1 if op == "ConsistentSymmetricGradient" else 2
    ctx, p = _stepped(product_lib, pos, mass, vel, boundary, ws.short_steps(boundary_penalty_term=pen, operator_discretization=op), steps, policy)
    try:
        got, want, _, wall = _same(ctx, p, boundary, label=(handler, pen, op, policy))
        st = _state(ctx, p)
        ent = wr.entries(wall, st.x, st.y, st.h)
        count = sum(e["has"].astype(int) for e in ent)
        d = np.concatenate([e["d"][e["has"]] for e in ent])
        assert got.n == len(mass) and got.n_elements == (4 if handler == "AnalyticOverestimate" else 1)
        assert ((d > 0) & (d < 1)).any() and ((d > -0.5) & (d < 0)).any() and ((d > -1) & (d < -0.5)).any() and (d <= -1).any()
        if handler == "AnalyticOverestimate":
            assert (count == 2).sum() >= 10 and min(got.n_entries) >= 100
            assert got.force[LEFT][0] < 0 < got.force[RIGHT][0] and got.force[FLOOR][1] < 0 < got.force[CEILING][1]   # every wall is pushed outwards
            assert all(n > 0 for n in got.normal)
        else:
            assert (count <= 1).all() and got.n_entries[0] >= 400 and got.normal[0] > 0
        assert sum(got.n_wet) > 0 and all(w <= n for w, n in zip(got.n_wet, got.n_entries))
        k = int(np.argmax(got.n_entries))
        value, pid = got.peak_pressure(k)
        has = ent[k]["has"]
        assert value == float(st.p[has].max()) and pid == int(np.flatnonzero(has & (st.p == st.p[has].max()))[0])
        if op == "ConsistentSymmetricGradient":                                # p_ib = p_i is in the coefficient: another result than without
            simple = wr.Wall(boundary, wall.lam, wall.dlam, wall.penalty, wall.eps, wall.rest, False)
            assert wr.result_bytes(wr.wall_load(st, simple)[1]) != bytes(got)
        fx, fy = got.total_force
        assert fx == float(sum(got.exact(k, "force_x") for k in range(got.n_elements))) and np.isfinite(fy)
    finally:
        ctx.close()


# ---- 2. no boundary -----------------------------------------------------------------------------------------------------------------
def test_a_context_without_planes_has_no_elements(product_lib):
    scn, pos, mass, vel = ws.small_scene(16, 8)
    ctx = ffi.Context(product_lib, len(mass) + 8, [])
    try:
        ctx.upload(mass, pos, vel)
        p = dam_break_params().to_ffi()
        got = wall_loads.wall_load(ctx, p)                                     # (before any step: nothing is read)
        assert bytes(got) == bytes(1232) == wr.result_bytes(wr.wall_load(_state(ctx, p), wr.Wall.of([], ws.luts(), p))[1])
        assert got.n_elements == 0 and got.force == [] and got.total_force == (0.0, 0.0)
        got = wall_loads.wall_load(ctx, p, 4, [FLOOR_RANGE])
        assert bytes(got) == bytes(1232) and got.words.shape == (0, 4)
    finally:
        ctx.close()


# ---- 3. d exactly 1, just below 1, exactly 0, exactly -1 and beyond; bins and their edges ------------------------------------------
@pytest.fixture(scope="module")
def placed(product_lib):
    """small_scene after one step, then twelve particles that carry pressure placed by hand (sph_upload_field behind the step: density
    and pressure stay): h = 2^-6, so sr = 2^-5 and every quotient below is exact."""
    scn, pos, mass, vel = ws.small_scene()
    ctx, p = _stepped(product_lib, pos, mass, vel, PLANES, dam_break_params(), 1)
    prs, h, x = ctx.download("pressure"), ctx.download("h2"), ctx.download("position")
    who = np.flatnonzero(prs > 0)[:12]
    assert len(who) == 12
    sr = f32(2.0 ** -5)
    h[who] = f32(2.0 ** -6)
    below = np.nextafter(f32(-1.0) + sr, f32(-2.0))
    # floor (plane 2): probe = y + 1.  0: d = 1 (no entry)  1: just below 1  2: d = 0  3: d = -1 (lambda = 1)  4: d = -2  5: just above -1
    ys = [f32(-1.0) + sr, below, f32(-1.0), f32(-1.0) - sr, f32(-1.0) - f32(2.0) * sr, np.nextafter(f32(-1.0) - sr, f32(0.0))]
    for j, y in enumerate(ys):
        x[who[j]] = (f32(0.25 + 0.125 * j), y)
    # bins on the floor, s = -x over [-2, 2): 6: on an edge of B = 4096 and B = 1 only  7: on s_lo (bin 0)  8: below s_lo  9: at s_hi
    # 10: on an edge of B = 7 (found below)  11: in the middle
    half = f32(-1.0) + f32(0.5) * sr
    x[who[6]] = (f32(-(-2.0 + 1500.0 / 1024.0)), half)
    x[who[7]] = (f32(2.0), half)
    x[who[8]] = (f32(2.5), half)
    x[who[9]] = (f32(-2.0), half)
    x[who[10]] = (f32(0.0), half)                                              # s + 2 = 2: 2 * 1.75 = 3.5 -> replaced below
    x[who[11]] = (f32(1.0), half)
    # an s whose (s - s_lo) * inv_ds is the integer 3 for B = 7 (inv_ds = 1.75; 12 / 7 is no float: look among the floats around it)
    cand = [f32(-2.0) + f32(3.0) * f32(4.0 / 7.0)]
    for _ in range(40):
        cand = [np.nextafter(cand[0], f32(-9.0))] + cand + [np.nextafter(cand[-1], f32(9.0))]
    on_edge = [s for s in cand if (s - f32(-2.0)) * f32(1.75) == f32(3.0)]
    assert on_edge, cand
    x[who[10], 0] = -on_edge[0]
    ctx.upload_field("h2", h)
    ctx.upload_field("position", x)
    yield ctx, p, who
    ctx.close()


def test_d_on_its_branch_points(placed):
    ctx, p, who = placed
    got, want, _, wall = _same(ctx, p, PLANES)
    st = _state(ctx, p)
    floor = wr.entries(wall, st.x, st.y, st.h)[FLOOR]
    d, has = floor["d"][who[:6]], floor["has"][who[:6]]
    # the twin sees the values the positions were built for (a case that misses its branch fails here)
    assert d[0] == 1.0 and not has[0]
    assert 0.999 < d[1] < 1.0 and has[1]
    assert d[2] == 0.0 and has[2] and d[3] == -1.0 and has[3] and d[4] == -2.0 and has[4] and -1.0 < d[5] < -0.999 and has[5]
    # lambda = 1, dlambda = 0 at and beyond d = -1: with Quadratic1, s = dpenalty * 1 + penalty * 0 = -1, g = -n / sr exactly
    sr = f32(2.0 ** -5)
    assert floor["gy"][who[3]] == floor["gy"][who[4]] == -f32(1.0) / sr and floor["gy"][who[5]] != floor["gy"][who[3]]
    assert got.n_entries[FLOOR] == int(floor["has"].sum())


@pytest.mark.parametrize("B", [1, 7, 4096])
def test_bins_and_their_edges(placed, B):
    ctx, p, who = placed
    ranges = [None, None, FLOOR_RANGE, None]
    got, want, prof, wall = _same(ctx, p, PLANES, B, ranges, label=B)
    st = _state(ctx, p)
    floor = want["elements"][FLOOR]
    b, s = wr.bin_of(wall, FLOOR, st.x[who], st.y[who], -2.0, floor["inv_ds"], B)
    assert floor["inv_ds"] == B / 4.0 and got.result.element[FLOOR].inv_ds == B / 4.0 and got.result.element[FLOOR].n_bins == B
    assert s[7] == -2.0 and b[7] == 0                                          # on s_lo: the first bin
    assert s[8] < -2.0 and b[8] == -1 and s[9] == 2.0 and b[9] == -1           # below s_lo and at s_hi: unbinned
    assert got.n_unbinned[FLOOR] == floor["n_unbinned"] >= 2
    edge = (s - f32(-2.0)) * f32(floor["inv_ds"])
    if B == 4096:
        assert edge[6] == 1500.0 and b[6] == 1500
    if B == 7:
        assert edge[10] == 3.0 and b[10] == 3
    # sum of the bins + the unbinned entries' terms = NORMAL once rescaled, in the twin's integers (the device's words are the twin's)
    e = floor["exponent"][wr.NORMAL]
    ent = wr.entries(wall, st.x, st.y, st.h)[FLOOR]
    t = wr.terms(st.m, wr.coefficient(wall, st.p, st.rho), st.x, st.y, ent)[wr.NORMAL][ent["has"]]
    assert int(got.words[FLOOR].sum()) + floor["unbinned_terms"] == sum(int(v * 2.0 ** (40 - e)) for v in t)
    assert abs((int(got.words[FLOOR].sum()) + floor["unbinned_terms"]) * 2 ** 20 - got.raw[FLOOR]["normal"]) < len(t) * 2 ** 20
    assert not got.words[[LEFT, RIGHT, CEILING]].any() and (got.words[FLOOR] != 0).sum() >= min(B, 3)
    centres, q = got.profile(FLOOR)
    assert len(centres) == B and centres[0] == -2.0 + 2.0 / B and np.array_equal(q, got.bin_forces(FLOOR) / (4.0 / B))
    assert got.profile(LEFT)[0].size == 0
    if B == 7:                                                                 # every plane its own range and bin count
        _same(ctx, p, PLANES, 7, [(-1.0, 1.0, 3), (-1.0, 1.0), (-2.0, 2.0, 5), (-2.0, 2.0, 1)], label="per plane")


# ---- 4. explicit versus automatic exponents ---------------------------------------------------------------------------------------
def test_explicit_and_automatic_exponents(placed):
    ctx, p, who = placed
    auto, want, _, _ = _same(ctx, p, PLANES)
    used = [e["exponent"] for e in want["elements"]]
    wider = [[e + 3 for e in row] for row in used]
    got, _, _, _ = _same(ctx, p, PLANES, exps=wider)
    assert [[got.exponents[k][s] for s in wr.SUMS] for k in range(4)] == wider
    for k in range(4):
        for s, name in enumerate(wr.SUMS):                                     # three more bits of headroom: the same number, coarser
            assert abs(got.sums[k][name] - auto.sums[k][name]) <= 2.0 ** (wider[k][s] - 60) * max(auto.n_entries[k], 1) + 2.0 ** -52 * abs(auto.sums[k][name])
    mixed = [None, [None, used[1][1] + 1, None, None], [5, None, None, used[2][3]], None]
    _same(ctx, p, PLANES, exps=mixed)
    _same(ctx, p, PLANES, 7, [None, None, FLOOR_RANGE, None], exps=wider)      # the bins follow e_NORMAL
    small = [None, None, [None, None, None, used[2][3] - 1], None]
    text = _refused(ctx, p, PLANES, exps=small)
    assert "sum 3 (normal) at element 2 is not finite or not below 2^exponent" in text
    _refused(ctx, p, PLANES, "exponent 201", exps=[[201, None, None, None]])
    _same(ctx, p, PLANES)                                                      # nothing changed


# ---- 5. more than one partial per lane of the fold launch -----------------------------------------------------------------------------
def test_multi_block_launch(product_lib):
    """sph_wall_load.hip: a streaming pass launches ceil(n / 256) blocks (at most 1024) and a fold launch folds their partials with
    kFoldWidth = 64 lanes: a lane folds more than one partial from 65 blocks on, i.e. from n = 256 * 64 + 1 = 16385 particles."""
    scn, pos, mass, vel = ws.small_scene(160, 104, 1.0 / 80)
    assert len(mass) >= 256 * 64 + 1 and (len(mass) + 255) // 256 > 64
    planes = sc.boundary_planes(scn.boundary)
    ctx, p = _stepped(product_lib, pos, mass, vel, planes, ws.short_steps(), 1)
    try:
        got, _, _, _ = _same(ctx, p, planes, 7, [(-1.0, 1.0), None, FLOOR_RANGE, None])
        assert got.n == len(mass) and got.n_entries[LEFT] >= 100 and got.n_entries[FLOOR] >= 150 and got.normal[FLOOR] > 0
        slots = ws.oh.device_slots(ctx.download("cell_index"))                  # the entries sit in many blocks of the device's order
        wall = wr.Wall.of(planes, ws.luts(), p)
        st = _state(ctx, p)
        ent = wr.entries(wall, st.x, st.y, st.h)
        assert len(np.unique(slots[ent[LEFT]["has"] | ent[FLOOR]["has"]] // 256)) > 8
    finally:
        ctx.close()


# ---- 6. order independence -----------------------------------------------------------------------------------------------------------
def test_shuffled_upload_gives_the_same_bytes(product_lib):
    """Isolated particles (nobody within anybody's support) along the floor and the left wall at jittered distances: a step treats each
    on its own, so two upload orders leave the same state particle for particle -- asserted -- and the loads must agree byte for byte,
    the peak's id permuted back."""
    rng = np.random.default_rng(11)
    m = f32(4e-4)
    sr = f32(2.0) * ws.h_of(m)
    along = np.arange(50, dtype=np.float64) * 1.5 * float(sr)
    floor = np.stack([-1.5 + along, -1.0 + rng.uniform(-1.2, 0.9, 50) * float(sr)], 1)
    left = np.stack([-2.0 + rng.uniform(-1.2, 0.9, 20) * float(sr), -0.5 + along[:20]], 1)
    free = np.stack([0.5 + along[:20], np.full(20, 0.3)], 1)
    pos = np.concatenate([floor, left, free]).astype(f32)
    n = len(pos)
    mass, vel = np.full(n, m, f32), np.zeros((n, 2), f32)
    perm = rng.permutation(n)
    P = ws.short_steps()
    a, p = _stepped(product_lib, pos, mass, vel, PLANES, P, 1)               # (a second step finds them flying off the wall: no pressure)
    b, _ = _stepped(product_lib, pos[perm], mass[perm], vel[perm], PLANES, P, 1)
    try:
        assert (a.download("neighbor_count") == 1).all()
        for f in ws.FIELDS:
            assert a.download(f)[perm].tobytes() == b.download(f).tobytes(), f
        ra, _, pa, _ = _same(a, p, PLANES, 7, [(-1.0, 1.0), None, FLOOR_RANGE, None])
        rb, _, pb, _ = _same(b, p, PLANES, 7, [(-1.0, 1.0), None, FLOOR_RANGE, None])
        assert ra.n_entries[FLOOR] >= 30 and ra.n_entries[LEFT] >= 12 and ra.n_wet[FLOOR] >= 5 and ra.words.tobytes() == rb.words.tobytes()
        for k in range(4):                                                     # ids permuted back for the peak key
            (va, ia), (vb, ib) = ra.peak_pressure(k), rb.peak_pressure(k)
            assert va == vb and (ia == ib == ffi.LEDGER_NO_ID or ia == perm[ib])
            rb.result.element[k].max_pressure.id = ia
        assert bytes(ra) == bytes(rb)
    finally:
        a.close()
        b.close()


# ---- 7. refusals; the call is read-only ----------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was(product_lib):
    """Context `a` is asked, refused and answered between its steps; context `b` gets the same uploads and steps and is never asked.
    Both end with every downloadable field and the neighbour lists bit for bit the same."""
    scn, pos, mass, vel = ws.small_scene()
    P = dam_break_params(level_estimation_method="EmptyAngle", maximum_surface_distance=0.2)
    p = P.to_ffi()
    a, b = (ffi.Context(product_lib, len(mass) + 8, PLANES) for _ in range(2))
    try:
        for c in (a, b):
            c.upload(mass, pos, vel)
        text = _refused(a, p, PLANES)                                          # before the first step: the density is 0
        assert text == "wall load: the density is not positive (particle i=0; before the first step the density is 0: the load exists behind sph_step)"
        for c in (a, b):
            c.step(p)
        _same(a, p, PLANES)
        bad = a.download("mass")
        bad[[300, 17]] = np.nan
        for c in (a, b):
            c.upload_field("mass", bad)
        assert _refused(a, p, PLANES) == "wall load: the mass is not finite (particle i=17)"
        for c in (a, b):
            c.upload_field("mass", mass)
        _same(a, p, PLANES)
        _refused(a, p, PLANES, "s_hi > s_lo", bins=4, ranges=[None, None, (1.0, 1.0), None])
        _refused(a, p, PLANES, "s_hi > s_lo", bins=4, ranges=[None, None, (1.0, -1.0), None])
        _refused(a, p, PLANES, "bins = 4097", bins=4097, ranges=[None, None, FLOOR_RANGE, None])
        _refused(a, p, PLANES, "n_bins = 5", bins=4, ranges=[None, None, (-2.0, 2.0, 5), None])
        spec, out = wall_loads.wall_load_spec(), ffi.SphWallLoadResult()
        B = ffi.C.byref
        assert product_lib.wall_load_compute(a.handle, None, B(spec), B(out), None) == 1
        assert product_lib.wall_load_compute(a.handle, B(p), None, B(out), None) == 1
        assert product_lib.wall_load_compute(a.handle, B(p), B(spec), None, None) == 1
        assert product_lib.wall_load_compute(None, B(p), B(spec), B(out), None) == 1
        spec.bins, spec.n_bins[2], spec.s_lo[2], spec.s_hi[2] = 4, 4, -2.0, 2.0
        assert product_lib.wall_load_compute(a.handle, B(p), B(spec), B(out), None) == 1      # bins without a profile to write to
        spec = wall_loads.wall_load_spec()
        spec.flags = 2
        with pytest.raises(ffi.SphError, match="unknown bits"):
            wall_loads.wall_load(a, p, spec)
        for c in (a, b):
            c.step(p)
        _same(a, p, PLANES, 7, [(-1.0, 1.0), None, FLOOR_RANGE, None])
        for c in (a, b):
            c.step(p)
        for f in EVERY:
            assert a.download(f).tobytes() == b.download(f).tobytes(), f
        (oa, ia), (ob, ib) = a.download_neighbors(), b.download_neighbors()
        assert np.array_equal(oa, ob) and np.array_equal(ia, ib)
        assert bytes(wall_loads.wall_load(a, p)) == bytes(wall_loads.wall_load(b, p))
    finally:
        a.close()
        b.close()
    # bins on a polygon
    c, _ = _stepped(product_lib, pos, mass, vel, POLYGON, dam_break_params(), 1)
    try:
        _refused(c, p, POLYGON, "bins on a polygon boundary", bins=4, ranges=[FLOOR_RANGE])
        _same(c, p, POLYGON)
    finally:
        c.close()
    # a slab context
    grp = D.make_loopback_group(product_lib, pos, mass, vel, PLANES, 2)
    try:
        with pytest.raises(ffi.SphError) as e:
            wall_loads.wall_load(grp[0], p)
        assert e.value.status == 30 and "slab contexts are not supported" in str(e.value)
    finally:
        for c in grp:
            c.close()


# ---- 8. the run subcommand ---------------------------------------------------------------------------------------------------------------
def test_run_wall_loads_writes_what_wall_load_returns(product_lib, tmp_path):
    from adaptive_sph_amd.__main__ import build_parser, run
    from adaptive_sph_amd.simulation import init_fluid_sim, init_simulation_params
    from adaptive_sph_amd.simulation_parameters import SimulationParams
    cfg = str(GOLDEN / "default-config.yaml")
    scene = tmp_path / "scene.yaml"
    scene.write_text("boundary:\n  type: box\n  width: 4\n  height: 2\nblocks:\n  - pos: [-1.97, -0.97]\n    size: [1.0, 0.8]\n    spacing: 0.025\n"
                     "    volume_fill_ratio: 1.2\n    velocity: [0, 0]\n")
    path, folder = tmp_path / "loads.csv", tmp_path / "profiles"
    args = build_parser().parse_args(["run", cfg, str(scene), "--max-steps", "4", "--without-adaptivity", "--wall-loads", str(path), "--wall-load-profile",
                                      str(folder), "--wall-load-bins", "8", "--vtk-every", "2"])
    assert (args.wall_loads, args.wall_load_every, args.wall_load_bins) == (str(path), 1, 8)
    assert run(args, lib=product_lib, out=io.StringIO()) == 4
    rows = list(csv.reader(path.open()))
    assert rows[0] == wall_loads.csv_columns(4) and len(rows) == 5 and [r[0] for r in rows[1:]] == ["1", "2", "3", "4"]
    assert sorted(f.name for f in folder.iterdir()) == ["wall-load-00002.csv", "wall-load-00004.csv"]
    # the same state again
    scn = sc.SceneConfig.from_yaml(str(scene))
    params = init_simulation_params(SimulationParams.from_yaml(cfg, None), scn)
    sim = init_fluid_sim(params, scn, lib=product_lib)
    p = params.to_ffi()
    try:
        for _ in range(4):
            dt = sim.single_step_without_adaptivity(p)
        load = wall_loads.wall_load(sim.ctx, p)
        assert rows[4] == wall_loads.csv_row(4, sim.time, dt, load)
        last = dict(zip(rows[0], rows[4]))
        assert float(last["normal_2"]) == load.normal[FLOOR] > 0 and float(last["fy_2"]) == load.force[FLOOR][1] < 0
        assert int(last["peak_id_2"]) == load.peak_pressure(FLOOR)[1] and int(last["n_wet_2"]) == load.n_wet[FLOOR] > 0
        prof = list(csv.reader((folder / "wall-load-00004.csv").open()))
        planes = sc.boundary_planes(scn.boundary)
        binned = wall_loads.wall_load(sim.ctx, p, 8, wall_loads.plane_ranges(planes, scn.boundary))
        assert prof == [list(r) for r in wall_loads.profile_rows(binned)] and len(prof) == 1 + 4 * 8
        # line pressure x bin width, summed = the normal force less the entries outside the range (the block bulges through the left wall)
        binned_force = sum(float(r[3]) for r in prof[1:] if r[0] == "2") * (4.0 / 8)
        if binned.n_unbinned[FLOOR] == 0:
            assert binned_force == pytest.approx(load.normal[FLOOR], rel=1e-5)   # (40 bits per term)
        else:
            assert 0.5 * load.normal[FLOOR] < binned_force < load.normal[FLOOR]
    finally:
        sim.close()
