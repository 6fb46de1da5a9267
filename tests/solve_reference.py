"""The pressure solve's residual statistics in the DEVICE's order, in numpy float32 (TEST-ONLY; no GPU), and the stop rule that reads them.

The device reduces sweep B's per-particle residuals in three stages, each in an order the code writes down (csrc/sph_sweeps.hip,
csrc/sph_device.h).  Slots are the positions of the cell-sorted array; logical block b owns slots 256 b .. 256 b + 255 whatever
workgroup ran it (blk = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3)), so the hardware's block order does not enter.

  1. solver_block_partial, per wave of 64 slots: the counts are ballots; wave_sum_dpp(cls == 0 ? err : 0) is row_shr 1, 2, 4, 8 inside
     the rows of 16 lanes (a lane without a source adds 0), row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3, lane 63
     read: with r_k the sum of row k at its lane 15, (r3 + r2) + (r1 + r0), every row a balanced tree over its 16 lanes
     ((a15 + a14) + (a13 + a12)) + ... .  Idle lanes (the array's tail) enter as class 3 and add 0.
  2. ... thread 0 then adds the block's four waves in index order: ((w0 + w1) + w2) + w3 -> partials[blk].
  3. solver_reduce_decide (one context, 256 threads): thread t starts from 0 and adds partials t, t + 256, t + 512, ... one at a time
     (a trip of the loop requests four and pads with zero partials); wave_sum = the __shfl_down tree, offsets 32 .. 1, lane 0 read;
     waves 0 .. 3 added in index order.

Every stage is simulated lane for lane with arrays (all waves at once); no library sum is taken of a float.  `order` replaces ONE stage
by another order of the same addends -- what tests/test_solve_reference.py uses to show that the order is visible in the bits on the
scenes the GPU tests run.  NOTE on what "another order" can be: stage 1 and the shuffle tree of stage 3 are BALANCED binary trees, and a
balanced tree read backwards (lanes or rows reversed) is its own mirror image -- float addition commutes, so the bits cannot change.
The other order of stage 1 is therefore a ROTATION of the rows ((r0 + r3) + (r2 + r1)); stages 2 and 3 are chains, which a reversal
does change.

max_err runs through the same networks with fmaxf (exact in any order: a self-check, tests/test_solve_reference.py).
"""
import numpy as np

F = np.float32
WAVE = 64
BLOCK = 256            # SWEEP_THREADS: slots per logical block = threads of solver_reduce_decide's workgroup
TRIP = 4 * BLOCK       # partials one trip of solver_reduce_decide's loop requests
CLS_NORMAL, CLS_SINGULAR, CLS_NEGATIVE, CLS_IDLE = 0, 1, 2, 3
ORDERS = (None, "rows-rotated", "waves-reversed", "partials-reversed")


def _dpp_wave(v, op, row_order=(0, 1, 2, 3)):
    """wave_sum_dpp / wave_max_nonneg_dpp of (waves, 64) float32 lanes: the value read from lane 63"""
    v = v.reshape(-1, 4, 16)[:, list(row_order), :].copy()
    for k in (1, 2, 4, 8):                      # row_shr:k -- lane l of a row receives lane l - k, lanes l < k receive `old` = 0
        src = np.zeros_like(v)
        src[:, :, k:] = v[:, :, :-k]
        v = op(v, src)
    src = np.zeros_like(v)                      # row_bcast:15, row mask 0xa: lane 15 of rows 0 / 2 into every lane of rows 1 / 3
    src[:, 1, :] = v[:, 0, 15:16]
    src[:, 3, :] = v[:, 2, 15:16]
    v = op(v, src)
    src = np.zeros_like(v)                      # row_bcast:31, row mask 0xc: lane 31 (row 1, lane 15) into every lane of rows 2 and 3
    src[:, 2, :] = v[:, 1, 15:16]
    src[:, 3, :] = v[:, 1, 15:16]
    v = op(v, src)
    return v[:, 3, 15]


def _shfl_wave(v, op):
    """wave_sum / wave_max of (waves, 64) lanes: the __shfl_down tree, offsets 32 .. 1 (a lane whose source is beyond lane 63 receives
    its own value); lane 0 is read"""
    v = v.copy()
    for o in (32, 16, 8, 4, 2, 1):
        src = v.copy()
        src[:, : WAVE - o] = v[:, o:]
        v = op(v, src)
    return v[:, 0]


def _chain(cols, op):
    """((c0 op c1) op c2) op ... over the columns of a (rows, k) array, one at a time"""
    t = cols[:, 0].copy()
    for k in range(1, cols.shape[1]):
        t = op(t, cols[:, k])
    return t


def device_residual_totals(err, cls, order=None):
    """err: per-slot residuals (float32), cls: per-slot classes (0 normal, 1 singular, 2 negative), both in SLOT order.
    -> (partials, totals): partials = dict of per-block arrays normal / singular / negative (uint32), sum_err / max_err (float32);
    totals = dict normal, singular, negative (int), sum_err, max_err (float32) as solver_reduce_decide leaves them in SolverCtrl."""
    assert order in ORDERS, order
    err = np.ascontiguousarray(err, dtype=F)
    cls = np.ascontiguousarray(cls).astype(np.uint8)
    n = len(err)
    assert cls.shape == (n,) and n > 0
    nblocks = (n + BLOCK - 1) // BLOCK
    e = np.zeros(nblocks * BLOCK, F)
    c = np.full(nblocks * BLOCK, CLS_IDLE, np.uint8)      # the tail's idle lanes: class 3
    e[:n], c[:n] = err, cls
    # ---- 1. per wave
    lanes = c.reshape(-1, WAVE)
    val = np.where(c == CLS_NORMAL, e, F(0)).astype(F).reshape(-1, WAVE)
    rows = (1, 2, 3, 0) if order == "rows-rotated" else (0, 1, 2, 3)
    w_sum = _dpp_wave(val, np.add, rows)
    w_max = _dpp_wave(np.abs(val), np.maximum, rows)
    w_cnt = [np.count_nonzero(lanes == k, axis=1).astype(np.uint32) for k in (CLS_NORMAL, CLS_SINGULAR, CLS_NEGATIVE)]
    # ---- 2. per block: thread 0 adds waves 0 .. 3
    per_block = lambda a: a.reshape(nblocks, BLOCK // WAVE)[:, ::-1] if order == "waves-reversed" else a.reshape(nblocks, BLOCK // WAVE)
    partials = dict(normal=_chain(per_block(w_cnt[0]), np.add), singular=_chain(per_block(w_cnt[1]), np.add),
                    negative=_chain(per_block(w_cnt[2]), np.add), sum_err=_chain(per_block(w_sum), np.add),
                    max_err=_chain(per_block(w_max), np.maximum))
    # ---- 3. one workgroup: thread t takes partials t, t + 256, ... ; shuffle tree ; waves 0 .. 3
    ntrips = (nblocks + TRIP - 1) // TRIP
    totals = {}
    for key, op in (("normal", np.add), ("singular", np.add), ("negative", np.add), ("sum_err", np.add), ("max_err", np.maximum)):
        p = partials[key]
        padded = np.zeros(ntrips * TRIP, p.dtype)         # (k < nparts ? partials[k] : zero)
        padded[:nblocks] = p
        per_thread = padded.reshape(-1, BLOCK).T          # [t, j] = partial t + 256 j
        if order == "partials-reversed":
            per_thread = per_thread[:, ::-1]
        acc = _chain(np.concatenate([np.zeros((BLOCK, 1), p.dtype), per_thread], axis=1), op)
        waves = _shfl_wave(acc.reshape(BLOCK // WAVE, WAVE), op)
        totals[key] = _chain(waves.reshape(1, -1), op)[0]
    for key in ("normal", "singular", "negative"):
        totals[key] = int(totals[key])
    return partials, totals


def model_avg_error(totals):
    """solve_stats (csrc/sph_step.hip): avg_error = sum_err / (float)normal of the last decided iteration, NaN without a normal particle"""
    return F(totals["sum_err"]) / F(totals["normal"]) if totals["normal"] > 0 else F(np.nan)


def oracle_stop(residual_density, max_avg_error, max_iters, normal, sum_err, it, rest_density, dt):
    """oracle/step.c, the end of the loop of iisph_pressure_iterations, in float32: the two `break`s of the residual mode, then max_iters"""
    with np.errstate(all="ignore"):
        avg = F(sum_err) / F(normal) if normal > 0 else F(np.nan)
        if residual_density:
            if normal == 0 or (np.abs(avg / F(rest_density)) < F(max_avg_error) and it > 1):
                return True
        else:
            if normal == 0 or (np.abs(avg) < F(max_avg_error) / F(dt) and it > 1):
                return True
    return it == max_iters


def predicted_stop(totals, it, rule, rest_density, dt):
    """The decision the device takes on iteration `it` from the model's totals: solver_stop_rule (csrc/sph_solve_rule.hpp), restated in
    float32 by oracle_stop.  rule = dict(residual_density, max_avg_error, max_iters)."""
    return oracle_stop(rule["residual_density"], rule["max_avg_error"], rule["max_iters"], totals["normal"], totals["sum_err"], it, rest_density, dt)


def measure_of_average(avg, residual_density, rest_density, dt):
    """(lhs, threshold_of): the left-hand side the rule compares -- |avg / rest_density| (density) or |avg| (divergence) -- and the function
    tolerance -> right-hand side, both in float32 exactly as solver_stop_rule forms them.  The rule stops when lhs < threshold_of(tol)."""
    if residual_density:
        return np.abs(F(avg) / F(rest_density)), lambda tol: F(tol)
    return np.abs(F(avg)), lambda tol: F(tol) / F(dt)


def stop_measure(totals, residual_density, rest_density, dt):
    return measure_of_average(model_avg_error(totals), residual_density, rest_density, dt)


def bracket_average(avg, residual_density, rest_density, dt):
    """(tol_go, tol_stop): ADJACENT float32 tolerances with lhs >= threshold(tol_go) -- the rule does not stop -- and
    lhs < threshold(tol_stop) -- it stops.  Density mode: the threshold IS the tolerance: tol_go = lhs ("on the bound"), tol_stop the
    next float32 above.  Divergence mode: the threshold tol / dt is a division, "on the bound" may not be representable: start at
    lhs * dt and walk to the adjacent pair whose thresholds bracket lhs (tol -> tol / dt is monotone)."""
    lhs, thr = measure_of_average(avg, residual_density, rest_density, dt)
    assert np.isfinite(lhs) and lhs > 0
    tol = F(lhs) if residual_density else F(lhs * F(dt))
    for _ in range(8):                                    # (a product and a quotient: at most a few ulps off)
        if lhs < thr(tol):
            tol = np.nextafter(tol, F(0))
    for _ in range(8):
        if not lhs < thr(np.nextafter(tol, F(np.inf))):
            tol = np.nextafter(tol, F(np.inf))
    go, stop = F(tol), np.nextafter(tol, F(np.inf))
    assert not lhs < thr(go) and lhs < thr(stop), (lhs, go, stop)
    return float(go), float(stop)


def bracketing_tolerances(totals, residual_density, rest_density, dt):
    return bracket_average(model_avg_error(totals), residual_density, rest_density, dt)


# ---- the device's visiting order (pure numpy; tests/test_gpu_bitexact.py re-exports these two) ---------------------------------------
def h_from_mass(mass, rest_density=1.0):
    """h_next_from_mass (simulation.rs:1865-1871) in f32: 1.9 sqrt((m / rho0) (1 / pi))"""
    vol = mass.astype(np.float32) / np.float32(rest_density)
    return np.float32(1.9) * np.sqrt(vol * np.float32(0.318309873342514038086), dtype=np.float32)


def device_order(pos, h):
    """The device's slot order for particles at `pos`: stable sort by the cell of the SORTING grid -- cell = the support 2 h of the
    smallest particle, cell index floor(x / cs) per axis (IEEE f32 division, neighborhood_search.rs:253-255), cells ordered x fastest
    (:383-395); ties keep the upload order."""
    cs = np.float32(2.0) * np.float32(h.min())
    cx = np.floor(pos[:, 0].astype(np.float32) / cs)
    cy = np.floor(pos[:, 1].astype(np.float32) / cs)
    return np.lexsort((cx, cy))


# ---- the scenes and the oracle runs the CPU and GPU tests of the decision share -----------------------------------------------------
# name -> (nx, ny, spacing): jittered dam-break columns (scene.dam_break_small) whose particle counts sit on the reduction's edges
SCENES = {
    "one-wave": (8, 7, 1.0 / 40),        # n = 56 <= 64: one wave, 8 idle lanes
    "tail-63": (23, 25, 1.0 / 40),       # n = 575 = 2 * 256 + 63: three blocks, the tail wave one lane short
    "blocks-7": (40, 40, 1.0 / 40),      # n = 1600 = 6 * 256 + 64: the last block holds one full wave and three idle ones; 7 blocks
    "xcd-2": (53, 53, 1.0 / 64),         # n = 2809: 11 blocks, grid 16, per_xcd = 2 -- the first size at which blk != blockIdx.x
    "trip-2": (513, 512, 1.0 / 512),     # n = 262 656 = 1026 * 256: 1026 partials, the second trip of solver_reduce_decide's loop
}
HUGE_TOL = 1e30                          # a tolerance every residual passes: that solve stops at iteration 2 (iter > 1)


SQUEEZE = 0.95                           # the lattice drawn together about its corner: density 0.93 / 0.95^2 > rest, so the density
                                         # solve's "normal" particles (p > 0) fill the whole array -- at rest spacing only the bottom
                                         # rows are, every partial behind them is zero, and no order of zeros is visible in a sum


def solve_scene(name, jitter=0.2, seed=3, squeeze=SQUEEZE):
    """(mass, pos, vel, planes) of scene `name`, in the DEVICE's visiting order (device_order)."""
    from adaptive_sph_amd import scene as sc
    nx, ny, spacing = SCENES[name]
    scn = sc.dam_break_small(nx, ny, spacing)
    pos, mass, vel = sc.init_particles(scn)
    assert len(mass) == nx * ny, (name, len(mass))
    rng = np.random.default_rng(seed)
    corner = pos.min(axis=0)
    pos = (corner + (pos - corner) * F(squeeze)).astype(F)
    pos = (pos + rng.uniform(-jitter, jitter, pos.shape).astype(F) * F(spacing)).astype(F)
    vel = rng.normal(0, 0.05, vel.shape).astype(F)
    perm = device_order(pos, h_from_mass(mass))
    return mass[perm], pos[perm], vel[perm], sc.boundary_planes(scn.boundary)


def solve_params(solver, max_iters, div_tol=0.0, dens_tol=0.0, **kw):
    """dam_break_params with one solver, one max_iters and the tolerances of its (up to) two solves"""
    from adaptive_sph_amd.workloads import dam_break_params
    return dam_break_params(pressure_solver_method=solver, max_iters=max_iters, hybrid_dfsph_max_avg_divergence_error=div_tol,
                            hybrid_dfsph_max_avg_density_error=dens_tol, iisph_max_avg_density_error=dens_tol, **kw)


def residual_mode(which):
    return 1 if which == "density" else 0


def solves_of(solver):
    return {"IISPH": ("density",), "OnlyDivergence": ("divergence",), "HybridDFSPH": ("divergence", "density")}[solver]


def forced_tolerances(solver, which):
    """the tolerances of an oracle step that FORCES solve `which` to max_iters: that solve's tolerance 0 -- and the other solve of
    HybridDFSPH stopped at iteration 2 by HUGE_TOL on both sides, whatever max_iters is (>= 2)"""
    other = HUGE_TOL if len(solves_of(solver)) == 2 else 0.0
    return dict(div_tol=0.0 if which == "divergence" else other, dens_tol=0.0 if which == "density" else other)


def oracle_step(oracle_lib, state, P):
    """a fresh oracle context, `state` = (mass, pos, vel, planes) uploaded, one step: (context, stats); the caller closes it"""
    from adaptive_sph_amd import ffi
    mass, pos, vel, planes = state
    o = ffi.Context(oracle_lib, len(mass), planes)
    o.upload(mass, pos, vel)
    return o, o.step(P.to_ffi())


def model_from_oracle(o, which):
    """The model's (partials, totals) of the last iteration of the last step's solve `which`, from the ORACLE's per-particle values.
    density: the field density_error, classes from aii and the final pressure (singular |aii| < 10e-4f; normal p > 0; else negative) --
    valid when the density solve is the step's last solve (it is, for every solver); divergence: oracle_solve_residuals."""
    if which == "density":
        err = o.download("density_error")
        aii, p = o.download("aii"), o.download("pressure")
        cls = np.where(np.abs(aii) < F(10e-4), CLS_SINGULAR, np.where(p > 0, CLS_NORMAL, CLS_NEGATIVE)).astype(np.uint8)
        res, cls2 = o.solve_residuals("density")   # (self-check: the entry point says the same)
        assert np.array_equal(cls, cls2) and np.array_equal(err[cls != CLS_SINGULAR].view(np.uint32), res[cls != CLS_SINGULAR].view(np.uint32))
    else:
        err, cls = o.solve_residuals("divergence")
    return device_residual_totals(err, cls)


def stats_of(st, which):
    return st.density_solver if which == "density" else st.div_solver


def forced_model(oracle_lib, state, solver, which, k, keep=False):
    """the oracle's step with solve `which` forced to k iterations -> (totals, stats, dt) [+ the live context when keep]"""
    o, so = oracle_step(oracle_lib, state, solve_params(solver, k, **forced_tolerances(solver, which)))
    assert int(stats_of(so, which).iters) == k, (solver, which, k, int(stats_of(so, which).iters))
    _, totals = model_from_oracle(o, which)
    s = stats_of(so, which)
    assert (totals["normal"], totals["negative"], totals["singular"]) == (int(s.normal_count), int(s.negative_count), int(s.singular_count))
    if keep:
        return totals, so, o
    o.close()
    return totals, so


def threshold_case(oracle_lib, state, solver, which, K, rest_density):
    """The adjacent tolerances around the model's value of iteration K of solve `which` (bracketing_tolerances), after asserting from the
    model on forced k = 2 .. K - 1 that no earlier iteration passes the looser of the two.  -> dict(go, stop, totals, dt)"""
    totals, so = forced_model(oracle_lib, state, solver, which, K)
    dt = float(so.dt)
    go, stop = bracketing_tolerances(totals, residual_mode(which), rest_density, dt)
    for k in range(2, K):
        tk, sk = forced_model(oracle_lib, state, solver, which, k)
        assert sk.dt == so.dt
        rule = dict(residual_density=residual_mode(which), max_avg_error=stop, max_iters=50)
        assert not predicted_stop(tk, k, rule, rest_density, dt), f"iteration {k} < {K} already passes the tolerance of iteration {K}"
    return dict(go=go, stop=stop, totals=totals, dt=dt)


# ---- the cases (shared by tests/test_solve_reference.py, which checks the constructions on the CPU, and tests/test_gpu_solve_decision.py)
SMALL = ("one-wave", "tail-63", "blocks-7", "xcd-2")
SOLVES = [("IISPH", "density"), ("OnlyDivergence", "divergence"), ("HybridDFSPH", "divergence"), ("HybridDFSPH", "density")]
FORCED_KS = (0, 1, 2, 5)
# (b) the decision at its threshold: (scene, solver, solve, K).  K = 2 is the first iteration the rule may stop at (no precondition);
# K = 5 (>= 4) on the 7-block scene, where threshold_case asserts that iterations 2 .. 4 do not pass; the 1026-partial scene once.
THRESHOLD_CASES = [(s, sv, w, 2) for s in SMALL for sv, w in SOLVES] + [("blocks-7", sv, w, 5) for sv, w in SOLVES[:2]] + [("trip-2", "IISPH", "density", 2)]
# (c) the predicted free-running count on the 7-block scene, three consecutive steps: (solver, solve, the tolerance of each step).  The
# scene relaxes quickly (the model's |avg / rho0| resp. |avg| dt at forced k = 2 .. 8, first step: IISPH 2.72e-2 2.06e-2 1.70e-2 1.43e-2
# 1.23e-2 1.08e-2 9.72e-3; OnlyDivergence 6.94e-4 5.02e-4 3.94e-4 3.17e-4 2.61e-4 2.20e-4 1.91e-4; the divergence residual falls fivefold
# over the three steps), so no single tolerance keeps K* in 4 .. 10 at all three: each step has its own, picked from the model's sequence
# of THAT step as the middle of the gap between two consecutive iterations, two or three digits -- percent, not ulps, away from both.
# The residuals are an order of magnitude above configs[1]'s (a jittered lattice drawn together): configs[1]'s own 0.002 / 0.001 would
# give K* ~ 30 / 2.
# The last entry records the K* the model finds (7 = "between k = 6 and k = 7"); the tests take K* from the model, not from here.
FREE_CASES = [("IISPH", "density", (0.0115, 0.0192, 0.0192), (7, 8, 4)), ("OnlyDivergence", "divergence", (2.4e-4, 1.12e-4, 6.3e-5), (7, 7, 7))]
FREE_STEPS = 3
MARGIN_ULPS = 4


def predicted_count(oracle_lib, state, solver, which, tol, rest_density, k_max=12):
    """K* = the first k >= 2 whose model totals (oracle forced to k) pass `tol` -> (K*, margin in ulps of the compared value at K* and
    at K* - 1 -- the smaller of the two, the oracle's context of the forced-K* step (live: the caller closes it), its stats)"""
    margins = []
    for k in range(2, k_max + 1):
        totals, so, o = forced_model(oracle_lib, state, solver, which, k, keep=True)
        dt = float(so.dt)
        lhs, thr = stop_measure(totals, residual_mode(which), rest_density, dt)
        margins.append(abs(float(lhs) - float(thr(tol))) / float(np.spacing(F(lhs))))
        rule = dict(residual_density=residual_mode(which), max_avg_error=tol, max_iters=50)
        if predicted_stop(totals, k, rule, rest_density, dt):
            return k, min(margins[-2:]), o, so
        o.close()
    raise AssertionError(f"the model does not stop within {k_max} iterations at tolerance {tol}")


def reordered(mass, pos, vel, planes):
    """the state in the device's visiting order of its CURRENT positions (what stepwise does before every step)"""
    perm = device_order(pos, h_from_mass(mass))
    return mass[perm], pos[perm], vel[perm], planes


def loners(nx=12, ny=6, spacing=1.0 / 40, apart=5.0):
    """nx * ny particles of the small scenes' mass on a lattice `apart` spacings wide around the origin: farther than a support
    (2 h = 2.07 spacings) from each other and from every wall of the 4 x 2 box, so every a_ii is 0: all singular.  In device order."""
    from adaptive_sph_amd import scene as sc
    scn = sc.dam_break_small(2, 2, spacing)
    _, mass1, _ = sc.init_particles(scn)
    gx, gy = np.meshgrid(np.arange(nx) - (nx - 1) / 2, np.arange(ny) - (ny - 1) / 2, indexing="ij")
    pos = (np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1) * (apart * spacing)).astype(F)
    mass = np.full(len(pos), mass1[0], F)
    rng = np.random.default_rng(5)
    vel = rng.normal(0, 0.05, pos.shape).astype(F)
    return reordered(mass, pos, vel, sc.boundary_planes(scn.boundary))
