"""The wall-load twin (tests/wall_load_reference.py, the restatement of include/sph_wall_load.h every device test compares with) against the
CPU oracle: its boundary entries ARE the step's, its coefficient times its entries IS the boundary part of the pressure acceleration, and
on a block at rest its floor carries the block's weight.  Then the twin's own refusals and exponent rules.  No GPU."""
import math

import numpy as np
import pytest

from adaptive_sph_amd import ffi, scene as sc
from adaptive_sph_amd.workloads import dam_break_params
from tests import ledger_reference as lr, wall_load_reference as wr, wall_load_scenes as ws

f32 = np.float32
# (boundary handler, penalty term): the four planes under each penalty term, and the polygon box
CASES = [("AnalyticOverestimate", pen) for pen in ws.PENALTIES] + [("AnalyticUnderestimate", "Quadratic1")]


def _one_step(oracle_lib, pos, mass, vel, boundary, P):
    ctx = ffi.Context(oracle_lib, len(mass) + 8, boundary)
    ctx.upload(mass, pos, vel)
    p = P.to_ffi()
    ctx.step(p)
    return ctx, p


def _per_particle_sums(ent, scale=None):
    """sum over the entries of every particle in SDF order, f32, from 0: (scale * gx, scale * gy)"""
    n = len(ent[0]["has"]) if ent else 0
    gx, gy, cnt = np.zeros(n, f32), np.zeros(n, f32), np.zeros(n, np.int64)
    for e in ent:
        ex, ey = (e["gx"], e["gy"]) if scale is None else ((scale * e["gx"]).astype(f32), (scale * e["gy"]).astype(f32))
        gx = np.where(e["has"], gx + ex, gx).astype(f32)
        gy = np.where(e["has"], gy + ey, gy).astype(f32)
        cnt += e["has"]
    return np.stack([gx, gy], axis=1), cnt


@pytest.fixture(scope="module")
def stepped(oracle_lib):
    """strays_scene after ONE oracle step, per case: (context, ffi params, twin wall, uploaded positions, the strays' indices)"""
    scn, pos, mass, vel, strays = ws.strays_scene()
    out = {}
    for handler, pen in CASES:
        for op in ("ConsistentSimpleGradient", "ConsistentSymmetricGradient"):
            boundary = sc.boundary_planes(scn.boundary, handler)
            ctx, p = _one_step(oracle_lib, pos, mass, vel, boundary, ws.short_steps(boundary_penalty_term=pen, operator_discretization=op))
            out[handler, pen, op] = (ctx, p, wr.Wall.of(boundary, ws.luts(), p), pos, strays)
    yield out
    for ctx, *_ in out.values():
        ctx.close()


# ---- 1. the twin's entry arithmetic is the step's ---------------------------------------------------------------------------------
@pytest.mark.parametrize("handler,pen", CASES)
def test_entries_are_the_steps(stepped, handler, pen):
    """The twin's entries at the UPLOADED positions with the step's h, summed per particle in SDF order in f32, equal the oracle's
    SPH_F_LAMBDA_GRAD_SUM (and the lambda sums its SPH_F_LAMBDA_SUM) bit for bit."""
    ctx, p, wall, pos, strays = stepped[handler, pen, "ConsistentSimpleGradient"]
    ent = wr.entries(wall, pos[:, 0], pos[:, 1], ctx.download("h2"))
    got, cnt = _per_particle_sums(ent)
    assert got.tobytes() == ctx.download("lambda_grad_sum").tobytes()
    lam = np.zeros(len(pos), f32)
    for e in ent:
        lam = np.where(e["has"], lam + e["lam"], lam).astype(f32)
    assert lam.tobytes() == ctx.download("lambda_sum").tobytes()
    # what the scene must exercise
    assert (cnt > 0).sum() > 400 and (got != 0).any()
    d = np.concatenate([e["d"][e["has"]] for e in ent])
    if handler == "AnalyticOverestimate":
        assert (cnt == 2).sum() >= 10 and len(ent) == 4                       # corners: two entries
        assert ((d > 0) & (d < 1)).any() and ((d > -0.5) & (d < 0)).any() and ((d > -1) & (d < -0.5)).any() and (d <= -1).any()
    else:
        assert len(ent) == 1 and (cnt <= 1).all() and (d < 0).any()           # one SDF: the polygon


# ---- 2. Newton's third law --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["ConsistentSimpleGradient", "ConsistentSymmetricGradient"])
@pytest.mark.parametrize("handler,pen", CASES)
def test_third_law_on_isolated_particles(stepped, handler, pen, op):
    """-sum_k c g_k of the twin at the step-start positions equals the oracle's SPH_F_PRESSURE_ACCEL on a particle whose neighbour list holds
    only itself (there the acceleration is the boundary term alone).  THE BAR THAT HOLDS: BIT FOR BIT -- the oracle's order is matched:
    f = -c, then r += f * g per entry from 0 (boundary_winchenbach2020.rs:164-194); negation is exact, so -(c g) and (-c) g are the same
    float."""
    ctx, p, wall, pos, strays = stepped[handler, pen, op]
    assert (ctx.download("neighbor_count")[strays] == 1).all()
    rho, prs = ctx.download("density"), ctx.download("pressure")
    ent = wr.entries(wall, pos[:, 0], pos[:, 1], ctx.download("h2"))
    c = wr.coefficient(wall, prs, rho)
    want, cnt = _per_particle_sums(ent, -c)
    got = ctx.download("pressure_accel")
    assert (cnt[strays] == 1).all()
    pushed = strays[prs[strays] > 0]
    assert len(pushed) >= 2 and (np.abs(got[pushed]).max(axis=1) > 0).all(), "no isolated particle is pushed by the wall: the test shows nothing"
    assert got[strays].tobytes() == want[strays].tobytes()
    if op == "ConsistentSymmetricGradient":                                   # p_ib = p_i really is in c
        simple = wr.Wall(wall.boundary, wall.lam, wall.dlam, wall.penalty, wall.eps, wall.rest, False)
        assert (wr.coefficient(simple, prs, rho)[pushed] < c[pushed]).all()


# ---- 3. hydrostatics --------------------------------------------------------------------------------------------------------------
# Measured on the CPU oracle (profiles/wall_loads.md): settled after 1000 steps, floor NORMAL / (total mass x g) = 0.9261, a deviation of
# 7.4 %.  That plus half of it again is 11.1 %; the bar stays at the 10 % it is not to exceed.  The side walls' FORCE_Y and the floor's
# FORCE_X measured EXACTLY 0 (an axis-aligned plane's central difference has one component that is exactly 0, and so has every entry's
# force): 0 plus half of it again is 0.
HYDROSTATIC_BAR = 0.10
BLOCK_STEPS, MAX_BLOCKS = 200, 20


def test_a_settled_block_weighs_on_the_floor(oracle_lib):
    scn = ws.resting_block_scene()
    pos, mass, vel = sc.init_particles(scn)
    assert 1000 < len(mass) <= 1500
    planes = sc.boundary_planes(scn.boundary)
    P = dam_break_params()
    p = P.to_ffi()
    ctx = ffi.Context(oracle_lib, len(mass) + 8, planes)
    try:
        ctx.upload(mass, pos, vel)
        wall = wr.Wall.of(planes, ws.luts(), p)
        weight = float(mass.astype(np.float64).sum()) * abs(float(p.gravity))
        kinetic, steps = [], 0
        while True:                                                           # until the ledger twin's kinetic energy has stopped falling
            for _ in range(BLOCK_STEPS):
                ctx.step(p)
            steps += BLOCK_STEPS
            state = lr.Particles({f: ctx.download(f) for f in ws.FIELDS + ["velocity"]}, None, P.rest_density)
            kind, led = lr.ledger(state, lr.CARRIED)
            assert kind == "ok"
            kinetic.append(led["sum"][lr.SUMS.index("kinetic")])
            if len(kinetic) > 1 and kinetic[-1] >= kinetic[-2]:
                break
            assert len(kinetic) < MAX_BLOCKS, kinetic
        kind, r, _ = wr.wall_load(state, wall)
        assert kind == "ok", r
        left, right, floor, ceiling = r["elements"]
        ratio = floor["sum"][wr.NORMAL] / weight
        print(f"settled after {steps} steps (kinetic energy {kinetic}): floor NORMAL / weight = {ratio:.4f}, side walls NORMAL / weight = "
              f"{left['sum'][wr.NORMAL] / weight:.4f}, {right['sum'][wr.NORMAL] / weight:.4f}; floor FORCE_X = {floor['sum'][wr.FORCE_X]!r}, side walls FORCE_Y = "
              f"{left['sum'][wr.FORCE_Y]!r}, {right['sum'][wr.FORCE_Y]!r}")
        assert len(kinetic) >= 3 and kinetic[-2] < kinetic[0]                   # it fell before it stopped falling
        assert abs(ratio - 1.0) <= HYDROSTATIC_BAR, ratio
        assert floor["sum"][wr.FORCE_Y] == -floor["sum"][wr.NORMAL] < 0         # the floor's normal is (0, 1) exactly: it is pushed down, fn = -fy
        assert floor["sum"][wr.FORCE_X] == 0.0 and left["sum"][wr.FORCE_Y] == 0.0 and right["sum"][wr.FORCE_Y] == 0.0
        assert left["sum"][wr.NORMAL] > 0 and right["sum"][wr.NORMAL] > 0 and ceiling["n_entries"] == 0
        assert floor["n_entries"] >= 40 and floor["n_wet"] > 0.8 * floor["n_entries"]
    finally:
        ctx.close()


# ---- 4. the twin's refusals and exponent rules --------------------------------------------------------------------------------------
def _state(n=64, seed=3):
    """particles along the floor of a 4 x 2 box, all with an entry there, pressures and densities as behind a step"""
    rng = np.random.default_rng(seed)
    h = f32(0.02)
    x = rng.uniform(-1.5, 1.5, n).astype(f32)
    y = (f32(-1.0) + rng.uniform(0.1, 1.5, n).astype(f32) * h).astype(f32)
    fields = {"mass": np.full(n, 4e-4, f32), "position": np.stack([x, y], 1), "density": rng.uniform(0.9, 1.1, n).astype(f32),
              "pressure": rng.uniform(0.0, 50.0, n).astype(f32), "h2": np.full(n, h, f32)}
    planes = sc.boundary_planes(sc.SceneBoundary("box", 4.0, 2.0))
    lam, dlam = ws.luts()
    return fields, wr.Wall(planes, lam, dlam, "Quadratic1", 1e-5, 1.0, False)


def _twin(fields, wall, ids=None, **kw):
    return wr.wall_load(lr.Particles(fields, ids, 1.0), wall, **kw)


def test_twin_refusals_name_the_smallest_id_and_the_first_reason():
    fields, wall = _state()
    kind, r, _ = _twin(fields, wall)
    assert kind == "ok" and r["elements"][2]["n_entries"] == 64 and r["n"] == 64
    for name, slot, value, text in (("mass", 40, np.nan, "the mass is not finite (particle i=40)"), ("position", 7, np.inf, "the x is not finite (particle i=7)"),
                                    ("h2", 9, np.nan, "the smoothing length is not finite (particle i=9)"),
                                    ("density", 12, -np.inf, "the density is not finite (particle i=12)"),
                                    ("pressure", 3, np.nan, "the pressure is not finite (particle i=3)"),
                                    ("h2", 5, 0.0, "the smoothing length is not positive (particle i=5)"),
                                    ("density", 6, -1.0, "the density is not positive (particle i=6; before the first step")):
        f = {k: v.copy() for k, v in fields.items()}
        if name == "position":
            f[name][slot, 0] = value
        else:
            f[name][slot] = value
        f["pressure"][50] = np.nan                                            # a later particle offends too: the smallest id is named
        kind, sentence, _ = _twin(f, wall)
        assert kind == "refused" and sentence.startswith("wall load: ") and text in sentence, sentence
    # the first failing check of ONE particle, in the header's order; ids travel with the particles
    f = {k: v.copy() for k, v in fields.items()}
    f["pressure"][20], f["position"][20, 1], f["density"][20] = np.nan, np.nan, 0.0
    kind, sentence, _ = _twin(f, wall, ids=np.arange(64)[::-1] + 100)
    assert sentence == "wall load: the y is not finite (particle i=143)"
    # before the first step every density is 0
    f = {k: v.copy() for k, v in fields.items()}
    f["density"][:] = 0.0
    kind, sentence, _ = _twin(f, wall)
    assert sentence == "wall load: the density is not positive (particle i=0; before the first step the density is 0: the load exists behind sph_step)"
    # finite inputs, a term that is not: rho * rho underflows to 0 in f32, c = inf, and fx = inf * 0 is no number -- sum 0 fails first
    f = {k: v.copy() for k, v in fields.items()}
    f["density"][33], f["pressure"][33] = 1e-30, 1.0
    kind, sentence, _ = _twin(f, wall)
    assert sentence == "wall load: the term of sum 0 (force_x) at element 2 is not finite (particle i=33)"


def test_twin_exponent_rules():
    fields, wall = _state()
    kind, auto, _ = _twin(fields, wall)
    floor = auto["elements"][2]
    assert [el["exponent"] for k, el in enumerate(auto["elements"]) if k != 2] == [[0] * 4] * 3          # no entries: exponent 0, integer 0
    assert all(el["raw"] == [0] * 4 and el["max_pressure"] == (0.0, lr.NO_ID) for k, el in enumerate(auto["elements"]) if k != 2)
    state = lr.Particles(fields, None, 1.0)
    t = wr.terms(state.m, wr.coefficient(wall, state.p, state.rho), state.x, state.y, wr.entries(wall, state.x, state.y, state.h)[2])
    for s in (wr.FORCE_Y, wr.TORQUE, wr.NORMAL):                               # the smallest e with max |t| < 2^e
        m = np.abs(t[s]).max()
        assert 2.0 ** (floor["exponent"][s] - 1) <= m < 2.0 ** floor["exponent"][s]
        assert floor["raw"][s] == sum(int(v * 2.0 ** (60 - floor["exponent"][s])) for v in t[s])
        assert abs(floor["sum"][s] - t[s].sum()) <= 64 * 2.0 ** (floor["exponent"][s] - 60) + 1e-15 * abs(t[s].sum())
    assert floor["exponent"][wr.FORCE_X] == 0 and floor["raw"][wr.FORCE_X] == 0 and floor["raw"][wr.FORCE_Y] == -floor["raw"][wr.NORMAL] < 0
    # explicit: three more bits of headroom give the same numbers, coarser; mixed explicit and automatic
    wider = [None, None, [e + 3 for e in floor["exponent"]], None]
    kind, r, _ = _twin(fields, wall, exps=wider)
    assert kind == "ok" and r["elements"][2]["exponent"] == wider[2]
    assert all(abs(a - b) <= 64 * 2.0 ** (e - 60) for a, b, e in zip(r["elements"][2]["sum"], floor["sum"], wider[2]))
    mixed = [None, None, [None, floor["exponent"][1] + 1, None, 5], [7, None, None, None]]
    kind, r, _ = _twin(fields, wall, exps=mixed)
    assert r["elements"][2]["exponent"] == [0, floor["exponent"][1] + 1, floor["exponent"][2], 5] and r["elements"][3]["exponent"] == [7, 0, 0, 0]
    # one too small: every particle whose term reaches 2^(e - 1) offends, the smallest id is named
    small = [None, None, [None, None, None, floor["exponent"][wr.NORMAL] - 1], None]
    kind, sentence, _ = _twin(fields, wall, exps=small)
    reach = np.flatnonzero(np.abs(t[wr.NORMAL]) >= 2.0 ** small[2][3])
    assert kind == "refused" and len(reach) >= 1
    assert sentence == f"wall load: the term of sum 3 (normal) at element 2 is not finite or not below 2^exponent = 2^{small[2][3]} (particle i={reach.min()})"
    # the bytes: sizes and the empty elements
    assert len(wr.result_bytes(auto)) == 1232 and wr.result_bytes(auto)[16 + 4 * 152:] == bytes(152 * 4)
    assert math.ldexp(float(floor["raw"][3]), floor["exponent"][3] - 60) == floor["sum"][3]


def test_twin_bins_add_up():
    fields, wall = _state(200, 5)
    kind, r, prof = _twin(fields, wall, bins=7, ranges=[None, None, (-1.0, 1.0), None])       # the floor's s = -x: some entries lie outside
    floor = r["elements"][2]
    assert kind == "ok" and prof.shape == (4, 7) and not prof[[0, 1, 3]].any()
    assert floor["n_bins"] == 7 and floor["inv_ds"] == 3.5 and 0 < floor["n_unbinned"] < 200
    # sum of the bins + the unbinned entries' terms = NORMAL once rescaled: the bins keep 40 bits of every term, the sum 60
    state = lr.Particles(fields, None, 1.0)
    t = wr.terms(state.m, wr.coefficient(wall, state.p, state.rho), state.x, state.y, wr.entries(wall, state.x, state.y, state.h)[2])[wr.NORMAL]
    e = floor["exponent"][wr.NORMAL]
    assert int(prof[2].sum()) + floor["unbinned_terms"] == sum(int(v * 2.0 ** (40 - e)) for v in t)
    assert abs((int(prof[2].sum()) + floor["unbinned_terms"]) * 2 ** 20 - floor["raw"][wr.NORMAL]) < 200 * 2 ** 20
