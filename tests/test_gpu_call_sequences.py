"""Call sequences: what the host may do BETWEEN two steps, and what the step driver carried across the boundary by then.

A step leaves the next one's header (hdr_ahead), the next one's neighbour build queued on a predicted grid and adopted at the next
step's start (sph_step.hip: queue_ahead_build -> Ahead), the incremental sort's mover count, the paced queue's iteration counts, the
level stash and lists_after behind.  include/sph_ffi.h lets the host call anything between two steps and pass other sph_params to every
step.  Each ROW below is one such sequence: four undisturbed steps (the merge and the queued build are in their steady state), the
intervention, three more steps -- on three runners that start from the same upload and receive the same calls and parameters:

  A  the product's path (the laboratory build with no switch set: test_the_laboratory_build_runs_the_products_defaults);
  B  its plain twin, created under SPH_AHEAD_BUILD=0: no build ever crosses a step boundary.  B must equal A BIT FOR BIT after every
     step behind the intervention: every field sph_download serves, the bits of dt, both solvers' iters and normal_count, n, and on the
     last step the CSR of sph_download_neighbors, order included;
  O  the CPU oracle, which has no cross-step shortcut at all: A against O with the helpers and tolerances of tests/test_gpu_parity.py
     (forced iteration counts, so both sides do the same work), n equal, and the classes of a classifying row equal to A's own download
     right behind sph_classify (a threshold flip between device and oracle stays out of it).

A read-only row also asserts that A's next step ADOPTED the queued build (launch counters), every row prints whether it did.  The rows
are data: test_the_oracle_runs_the_row runs each of them without a GPU, the oracle in all three places, which checks the calls, the
scenes' own assertions and the list of rows the oracle refuses before anything goes to a device.

Scenes, the smallest that still take the shortcuts (the control rows prove it on the profile: A queued and adopted, B never did):
  block  the compressed block of test_iisph2_solver at its own size, 28 x 24 particles at 1.06 rho_0 (it reaches the steady state: no
         enlargement was needed), with the level radii of its with_classes case where a row classifies or reads level values;
  two    two_sizes_scene() of test_gpu_incremental_sort.py: ~2 000 particles, tiles, two smoothing lengths -- the rows that touch lists,
         tiles and support_length_estimation.
"""
from dataclasses import dataclass, field as dc_field
from functools import lru_cache
from pathlib import Path
from typing import Callable, Dict, Optional

import numpy as np
import pytest

from adaptive_sph_amd import adaptivity as A, ffi, render as R, scene as sc
from tests.test_gpu_adaptivity import decisions
from tests.test_gpu_incremental_sort import two_sizes_scene
from tests.test_gpu_parity import ALL_FIELDS, REL_TOL_FIELDS, TOL, forced, rel_err
from tests.test_gpu_partner_problem import all_fields, same_fields

REPO = Path(__file__).resolve().parent.parent
PATTERNS = REPO / "tests" / "golden" / "split-patterns.yaml"

# Rows the CPU oracle refuses (its status for a combination it does not implement): they keep their A == B comparison.  A row listed
# here MUST be refused by the oracle -- the run asserts it -- so the list cannot grow into a way around the comparison.
ORACLE_REFUSED = []

STEPS_BEFORE, STEPS_AFTER = 4, 3
STEPS = STEPS_BEFORE + STEPS_AFTER
AVAILABLE = ffi.MERGE_PARTNER_AVAILABLE


# ---- scenes and base parameters ----------------------------------------------------------------------------------------------------
def block_scene():
    s = 1 / 28
    return sc.SceneConfig(sc.SceneBoundary("box", 4.0, 2.0),
                          [sc.SceneFluidBlock([-2 + s, -1 + s], [28 * s + 0.5 * s, 24 * s + 0.5 * s], s, 1.06, [-0.5, 0.0])])


BLOCK = dict(max_iters=4, pressure_solver_method="IISPH", max_dt=0.0005)
BLOCK_LEVEL = dict(BLOCK, level_estimation_method="EmptyAngle", maximum_surface_distance=0.3, particle_radius_fine=0.016, particle_radius_base=0.022)
TWO = dict(max_iters=4)
TWO_LEVEL = dict(TWO, level_estimation_method="EmptyAngle", maximum_surface_distance=0.2, particle_radius_fine=0.004, particle_radius_base=0.02)
TWO_LEVEL_AFTER = dict(TWO_LEVEL, level_estimation_after_advection=True)
SCENES = {"block": block_scene, "two": two_sizes_scene}


# ---- a row ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class Row:
    name: str
    scene: str
    base: dict
    acts: Dict[int, Callable] = dc_field(default_factory=dict)   # step index -> the host's calls in front of that step (all runners)
    switch: Optional[dict] = None      # parameter overrides from the intervention on ...
    back: bool = False                 # ... and the first values again for the last step
    read_only: bool = False            # the calls change nothing a download can see (checked on A), and A's next step adopts the queued build
    classes: bool = False              # the classes behind sph_classify survive the following steps
    initial_classes: bool = False      # a patterned class field uploaded right behind sph_upload (rows that export partner candidates)
    control: bool = False


class Env:
    """What an intervention sees: the live runners, the parameters in force, the oracle's last dt."""

    def __init__(self, ctxs, P, planes, device=True):
        self.ctxs, self.P, self.planes, self.device = ctxs, P, planes, device
        self.p = P.to_ffi()
        self.dt = 0.0
        self.classes_after = None
        self.notes = []

    def each(self, needs=(), optional=False):
        """The runners that have the entry points `needs` (the oracle has no device, profiler, renderer or candidate export).  A device
        library has them all -- a row must not turn into no call at all -- except the renderer (`optional`)."""
        served = [c for c in self.ctxs.values() if all(getattr(c.lib, s, None) is not None for s in needs)]
        assert optional or not self.device or (self.ctxs["A"] in served and self.ctxs["B"] in served), needs
        return served

    @property
    def o(self):
        return self.ctxs["O"]

    def ap(self):
        return A.adapt_params(self.P, self.dt)


@lru_cache(maxsize=None)
def split_patterns():
    return A.SplitPatterns.load_from_file(PATTERNS)


# ---- interventions: read-only by contract -----------------------------------------------------------------------------------------
def ro_download_every_field(e):
    for c in e.each():
        all_fields(c)


def ro_download_neighbors(e):
    for c in e.each():
        c.download_neighbors()


def ro_grid(e):
    for c in e.each():
        c.grid()


def ro_sum_mass(e):
    for c in e.each(("sum_mass",)):
        assert c.sum_mass() > 0


def ro_partner_candidates(e):
    for c in e.each(("download_partner_candidates",)):
        tot = sum(len(c.download_partner_candidates(kind, e.p, e.ap())[1]) for kind in ("share", "merge"))
        assert tot > 0   # (the patterned classes leave donors with candidates)


def ro_partner_problem(e):
    for c in e.each(ffi.PROBLEM_SYMBOLS):
        tot = sum(len(c.download_partner_problem(kind, e.p, e.ap(), want_ids=True)[0]) for kind in ("share", "merge"))
        assert tot > 0


def ro_find_partners(e):
    for c in e.each(ffi.SEARCH_SYMBOLS):
        for kind in ("share", "merge"):
            info = c.find_partners_device(kind, e.p, e.ap())
            assert info["participants"] > 0
            c.download_partner_decisions(info["participants"])


def ro_render(e):
    for c in e.each(("render",), optional=True):
        img = R.render(c, e.P, R.VisualizationParams("Density"), 96, 64, planes=e.planes)
        assert img.shape == (64, 96, 3) and img.std() > 0


def ro_profile(e):
    for c in e.each(("profile_get", "profile_reset")):
        assert c.profile_get()
        c.profile_reset()


def ro_set_split_patterns(e):
    sp = split_patterns()
    for c in e.each():
        c.set_split_patterns(sp.patterns)


# ---- interventions: classification -----------------------------------------------------------------------------------------------
def classify(e):
    for c in e.each():
        c.classify(e.p)
    e.classes_after = {tag: c.download("particle_size_class").copy() for tag, c in e.ctxs.items()}
    a, o = e.classes_after["A"], e.classes_after.get("O")
    cnt = np.bincount(a, minlength=5)
    assert (cnt > 10).sum() >= 2, cnt     # the classes say something: not everyone is Optimal (what a stale array would hold)
    assert (a != A.OPTIMAL).sum() > 10, cnt
    if o is not None:
        e.notes.append(f"classes {cnt.tolist()}, device/oracle threshold flips: {int((a != o).sum())}")


def classify_split_nobody(e):
    sp = split_patterns()
    for c in e.each():
        c.set_split_patterns(sp.patterns)
    classify(e)
    assert not any((v == A.TOO_LARGE).any() for v in e.classes_after.values())
    n0 = e.ctxs["A"].n
    for c in e.each():
        c.split_particles(e.p, e.ap())
        assert c.n == n0


def classify_then_all_available(kind):
    def act(e):
        classify(e)
        for c in e.each():
            mp, mc = np.full(c.n, AVAILABLE, np.uint32), np.zeros(c.n, np.uint16)
            (c.share_particles if kind == "share" else c.merge_particles)(e.p, e.ap(), mp, mc)
    return act


# ---- interventions: writers (values taken ONCE, from the oracle's state, and handed to every runner) -----------------------------------
def third(n):
    return np.arange(n) % 3 == 1


def upload_of(name, edit):
    def act(e):
        v0 = e.o.download(name)
        v = v0.copy()
        w = edit(v)
        v = v if w is None else w
        assert not np.array_equal(v.view(np.uint8), v0.view(np.uint8))   # (the upload changes the state)
        for c in e.each():
            c.upload_field(name, v)
    return act


def _scale_third(f):
    def edit(v):
        v[third(len(v))] *= np.float32(f)
    return edit


def _shift_position(v):
    v += np.array([0.25, 0.1], np.float32)     # several cells (a cell is about two smoothing lengths ~ 0.1): another grid origin


def _fast_velocity(v):
    v[:, 0] += np.float32(60.0)                # the CFL term limits dt now: a stale header would show in dt


def _add_third(d):
    def edit(v):
        v[third(len(v))] += np.float32(d)      # (a NaN -- no level value -- stays one)
    return edit


def _class_pattern(v):
    return ((np.arange(len(v)) * 7) % 5).astype(np.uint8)


def edits_set(e):
    m, v = e.o.download("mass"), e.o.download("velocity")
    ops = [("set", i, {"mass": float(m[i]) * 1.02, "velocity": [float(v[i, 0]) + 0.3, float(v[i, 1]) - 0.2]}) for i in (0, 17, 333, e.o.n - 1)]
    for c in e.each():
        c.apply_edits(ops)


def edits_swap(e):
    ops = [("swap", 3, e.o.n - 5), ("swap", 100, 101)]
    for c in e.each():
        c.apply_edits(ops)


def edits_truncate(e):
    n_new = e.o.n - 5
    for c in e.each():
        c.apply_edits([("truncate", n_new)])
        assert c.n == n_new


def edits_extend_set(e):
    """Two new particles one spacing above the block's top row, with the values of the particles below them."""
    o = e.o
    n, x = o.n, o.download("position")
    f = {k: o.download(k) for k in ("mass", "velocity", "h2", "h2_next", "level_estimation", "level_old")}
    top = np.argsort(x[:, 1])[-2:]
    ops = [("extend", 2)]
    for k, i in enumerate(top):
        val = {"mass": float(f["mass"][i]), "position": [float(x[i, 0]), float(x[i, 1]) + 1 / 28], "velocity": [float(f["velocity"][i, 0]), float(f["velocity"][i, 1])],
               "h2": float(f["h2"][i]), "h2_next": float(f["h2_next"][i]), "level_old": float(f["level_old"][i])}
        if np.isfinite(f["level_estimation"][i]):
            val["level_estimation"] = float(f["level_estimation"][i])
        ops.append(("set", n + k, val))
    for c in e.each():
        c.apply_edits(ops)
        assert c.n == n + 2


def transfer_with_oracle_decisions(kind):
    def act(e):
        for c in e.each():
            c.classify(e.p)
        cls, off, idx, mp, mc = decisions(e.o, kind, e.P, e.p, e.dt)
        assert mc.sum() >= 5, (np.bincount(cls, minlength=5), mc.sum())
        n0 = e.o.n
        for c in e.each():
            c.upload_field("particle_size_class", cls)      # the oracle's classes on every side: the decisions are about them
            (c.share_particles if kind == "share" else c.merge_particles)(e.p, e.ap(), mp, mc)
        assert (e.o.n < n0) == (kind == "merge")
    return act


def split_with_oracle_classes(e):
    sp = split_patterns()
    e.o.classify(e.p)
    lvl, cls = e.o.download("level_estimation"), e.o.download("particle_size_class")
    assert (cls == A.TOO_LARGE).sum() >= 5, np.bincount(cls, minlength=5)
    n0 = e.o.n
    for c in e.each():
        c.set_split_patterns(sp.patterns)
        c.upload_field("level_estimation", lvl)   # identical inputs for num_children = round(mass / target_mass)
        c.upload_field("particle_size_class", cls)
        c.split_particles(e.p, e.ap())
    assert e.o.n > n0


def upload_reversed(e):
    m, x, v = (e.o.download(k)[::-1].copy() for k in ("mass", "position", "velocity"))
    for c in e.each():
        c.upload(m, x, v)


def set_time(e):
    for c in e.each():
        c.set_time(0.5, 100)


def refused_step(e):
    """A step every runner refuses before it launches anything (level estimation before advection without the extended range:
    simulation.rs:2018-2031): the context stays as it was (include/sph_ffi.h), what the last step left for the next one included."""
    bad = e.P.replace(use_extended_range_for_level_estimation=False).to_ffi()
    for c in e.each():
        with pytest.raises(ffi.SphError) as err:
            c.step(bad)
        assert err.value.status == 1   # SPH_ERR_INVALID_ARGUMENT


def policy(name):
    def act(e):
        for c in e.each():
            c.set_math_policy(name)
    return act


# ---- the rows ------------------------------------------------------------------------------------------------------------------------
def at(act):
    return {STEPS_BEFORE: act}


def _rows():
    rows = [Row("control-block", "block", BLOCK_LEVEL, control=True), Row("control-two", "two", TWO, control=True)]
    # read-only by contract
    rows += [Row("ro-download-every-field", "two", TWO, at(ro_download_every_field), read_only=True),
             Row("ro-download-neighbors", "two", TWO, at(ro_download_neighbors), read_only=True),
             Row("ro-grid", "two", TWO, at(ro_grid), read_only=True),
             Row("ro-sum-mass", "two", TWO, at(ro_sum_mass), read_only=True),
             Row("ro-partner-candidates", "block", BLOCK_LEVEL, at(ro_partner_candidates), read_only=True, initial_classes=True),
             Row("ro-partner-problem", "block", BLOCK_LEVEL, at(ro_partner_problem), read_only=True, initial_classes=True),
             Row("ro-find-partners-device", "block", BLOCK_LEVEL, at(ro_find_partners), read_only=True, initial_classes=True),
             Row("ro-render-frame", "two", TWO, at(ro_render), read_only=True),
             Row("ro-profile-get-reset", "two", TWO, at(ro_profile), read_only=True),
             Row("ro-set-split-patterns", "block", BLOCK_LEVEL, at(ro_set_split_patterns), read_only=True)]
    # classification
    for solver in ("IISPH", "HybridDFSPH"):
        base = dict(BLOCK_LEVEL, pressure_solver_method=solver)
        rows += [Row(f"classify-alone-{solver}", "block", base, at(classify), classes=True),
                 Row(f"classify-then-IISPH2-after-{solver}", "block", base, at(classify), dict(pressure_solver_method="IISPH2"), classes=True)]
    rows += [Row("classify-split-nobody-too-large", "block", BLOCK_LEVEL, at(classify_split_nobody), dict(pressure_solver_method="IISPH2"), classes=True),
             Row("classify-share-all-available", "block", BLOCK_LEVEL, at(classify_then_all_available("share")), dict(pressure_solver_method="IISPH2"), classes=True),
             Row("classify-merge-all-available", "block", BLOCK_LEVEL, at(classify_then_all_available("merge")), dict(pressure_solver_method="IISPH2"), classes=True)]
    # writers
    rows += [Row("upload-mass", "block", BLOCK, at(upload_of("mass", _scale_third(1.01)))),
             Row("upload-position", "block", BLOCK, at(upload_of("position", _shift_position))),
             Row("upload-velocity", "block", BLOCK, at(upload_of("velocity", _fast_velocity))),
             Row("upload-h2", "two", TWO, at(upload_of("h2", _scale_third(1.1)))),
             Row("upload-h2_next", "two", TWO, at(upload_of("h2_next", _scale_third(1.1)))),
             Row("upload-level_estimation", "block", BLOCK_LEVEL, at(upload_of("level_estimation", _add_third(0.01)))),
             Row("upload-level_old", "block", BLOCK_LEVEL, at(upload_of("level_old", _add_third(0.01)))),
             Row("upload-particle_size_class", "block", BLOCK_LEVEL, at(upload_of("particle_size_class", _class_pattern)), dict(pressure_solver_method="IISPH2")),
             Row("edits-set", "block", BLOCK, at(edits_set)),
             Row("edits-swap", "block", BLOCK, at(edits_swap)),
             Row("edits-truncate", "block", BLOCK, at(edits_truncate)),
             Row("edits-extend-set", "block", BLOCK, at(edits_extend_set)),
             Row("share-oracle-decisions", "block", dict(BLOCK_LEVEL, **RADII_SHARE), at(transfer_with_oracle_decisions("share"))),
             Row("merge-oracle-decisions", "block", dict(BLOCK_LEVEL, **RADII_MERGE), at(transfer_with_oracle_decisions("merge"))),
             Row("split-oracle-classes", "block", dict(BLOCK_LEVEL, **RADII_SPLIT), at(split_with_oracle_classes)),
             Row("upload-reversed", "two", TWO, at(upload_reversed)),
             Row("set-time", "two", TWO, at(set_time)),
             Row("refused-step", "two", TWO_LEVEL, at(refused_step), read_only=True)]
    # parameter switches
    solvers = ("IISPH", "IISPH2", "HybridDFSPH", "OnlyDivergence")
    rows += [Row(f"solver-{a}-to-{b}", "block", dict(BLOCK, pressure_solver_method=a), switch=dict(pressure_solver_method=b)) for a in solvers for b in solvers if a != b]
    rows += [Row("level-None-to-EmptyAngle", "two", dict(TWO_LEVEL, level_estimation_method="None"), switch=dict(level_estimation_method="EmptyAngle")),
             Row("level-EmptyAngle-to-None", "two", TWO_LEVEL, switch=dict(level_estimation_method="None")),
             # (CenterDiff needs density values: legal after advection only, simulation.rs:2029-2031)
             Row("level-EmptyAngle-to-CenterDiff", "two", TWO_LEVEL_AFTER, switch=dict(level_estimation_method="CenterDiff")),
             Row("level-after-advection-on-and-back", "two", TWO_LEVEL, switch=dict(level_estimation_after_advection=True), back=True),
             # (without the extended range the level estimation replays the step's lists: legal after advection only, simulation.rs:2018-2020)
             Row("level-extended-range-off", "two", TWO_LEVEL_AFTER, switch=dict(use_extended_range_for_level_estimation=False)),
             Row("support-length-Clamped1-and-back", "two", TWO, switch=dict(support_length_estimation="FromDistributionClamped1"), back=True),
             # (on the block nobody has more than 19 neighbours, so no smoothing length shrinks and the reference's `h_next < h` assertion
             #  stays quiet -- two_sizes_scene() trips it at once, on every runner; the switch still takes the step through its other path:
             #  per-pair smoothing lengths, h2_next := h2, no header and no build left for the next step)
             Row("constrain-neighborhood-count-on-and-back", "block", BLOCK, switch=dict(constrain_neighborhood_count=True), back=True),
             Row("rest-density-1.02", "block", BLOCK, switch=dict(rest_density=1.02)),
             Row("viscosity-type-WCSPH", "block", BLOCK, switch=dict(viscosity_type="WCSPH")),
             Row("operator-ConsistentSymmetricGradient", "block", BLOCK, switch=dict(operator_discretization="ConsistentSymmetricGradient")),
             Row("operator-Winchenbach2020", "two", TWO, switch=dict(operator_discretization="Winchenbach2020")),
             Row("boundary-penalty-Linear", "block", BLOCK, switch=dict(boundary_penalty_term="Linear")),
             Row("max-dt-halved", "block", BLOCK, switch=dict(max_dt=0.00025)),
             Row("max-iters-4-to-7", "block", BLOCK, switch=dict(max_iters=7)),
             Row("fill-stash-first-iteration", "block", BLOCK_LEVEL, switch=dict(fill_stash_with="SurfaceDistanceFirstIteration")),
             Row("gravity", "block", BLOCK, switch=dict(gravity=-4.0)),
             Row("pull-fluid-to", "block", BLOCK, switch=dict(pull_fluid_to=[0.0, 0.5, 0.0]))]
    # math policy: FAST -> EXACT (one step) -> FAST
    rows += [Row("policy-fast-exact-fast", "two", TWO, {STEPS_BEFORE: policy("exact"), STEPS_BEFORE + 1: policy("fast")})]
    return rows


# Radii (and, for sharing, a surface distance) that put the block's particles -- one mass, the level value grows from the surface inwards
# up to maximum_surface_distance -- on the sides of the class thresholds a transfer needs: sharing ~47 Large donors beside Small
# receivers in the steep band under the surface, merging the 240 TooSmall donors the interior holds (its level value is one value, so
# it changes class as a whole), splitting ~100 TooLarge particles under the surface.
RADII_SHARE = dict(maximum_surface_distance=0.08, particle_radius_fine=0.012, particle_radius_base=0.030)
RADII_MERGE = dict(particle_radius_fine=0.016, particle_radius_base=0.030)
RADII_SPLIT = dict(particle_radius_fine=0.012, particle_radius_base=0.026)
ROWS = _rows()
assert len({r.name for r in ROWS}) == len(ROWS)
assert set(ORACLE_REFUSED) <= {r.name for r in ROWS}


# ---- running a row -------------------------------------------------------------------------------------------------------------------
def stats_bits(st):
    return (np.float32(st.dt).view(np.uint32).item(), int(st.div_solver.iters), int(st.div_solver.normal_count),
            int(st.density_solver.iters), int(st.density_solver.normal_count), int(st.n_particles))


def step_each(ctxs, p):
    """Step every live runner: tag -> its stats, or the status it refused the step with."""
    out = {}
    for tag, c in ctxs.items():
        try:
            out[tag] = c.step(p)
        except ffi.SphError as err:
            out[tag] = int(err.status)
    return out


def launches(prof, name):
    return prof.get(name, (0, 0))[0]


def run_row(row, lib_a, lib_b, lib_o, monkeypatch, device=True):
    """`device=False`: A and B are no device libraries (the oracle in their place runs every row's calls on the CPU): no launch counters,
    none of the product-only entry points."""
    profile = device
    scn = SCENES[row.scene]()
    pos, mass, vel = sc.init_particles(scn)
    P0 = forced(**row.base)
    P1 = P0.replace(**row.switch) if row.switch else P0
    planes = sc.boundary_planes(scn.boundary, P0.init_boundary_handler)
    cap = 4 * len(mass)
    ctxs = {"A": ffi.Context(lib_a, cap, planes)}
    monkeypatch.setenv("SPH_AHEAD_BUILD", "0")      # (the switches are read at sph_create)
    ctxs["B"] = ffi.Context(lib_b, cap, planes)
    monkeypatch.delenv("SPH_AHEAD_BUILD")
    ctxs["O"] = ffi.Context(lib_o, cap, planes)
    e = Env(ctxs, P0, planes, device)
    profiled = [ctxs["A"], ctxs["B"]] if profile else []
    for c in ctxs.values():
        c.upload(mass, pos, vel)
        if row.initial_classes:
            c.upload_field("particle_size_class", _class_pattern(mass))
    for c in profiled:
        c.profile_enable(1)
    oracle_refused = False
    for s in range(STEPS):
        e.P = P0 if (s < STEPS_BEFORE or (row.back and s == STEPS - 1)) else P1
        e.p = e.P.to_ffi()
        if s in row.acts:
            before = all_fields(ctxs["A"]) if row.read_only else None
            row.acts[s](e)
            if row.read_only:
                same_fields(before, all_fields(ctxs["A"]))
        a = ctxs["A"]
        prof0 = a.profile_get() if profile and s == STEPS_BEFORE else None
        st = step_each(ctxs, e.p)
        if prof0 is not None:
            prof1 = a.profile_get()
            own = launches(prof1, "sort_scatter") - launches(prof0, "sort_scatter")
            print(f"[{row.name}] the step behind the intervention: sort_scatter +{own}, inc_reorder +{launches(prof1, 'inc_reorder') - launches(prof0, 'inc_reorder')}"
                  f" -> {'a build of its own' if own else 'adopted the queued build'}; {'; '.join(e.notes)}")
            if row.read_only:   # nothing was written: the build the last step queued is still the next step's
                assert own == 0, (prof0, prof1)
        # every step of a row is a legal one: a row that ended here would pass without having compared anything.  Only the oracle may
        # refuse (a combination it does not implement), and only in a row that says so.
        for tag in ("A", "B"):
            assert not isinstance(st[tag], int), f"[{row.name}] step {s}: {tag} refused the step: {ffi.STATUS_NAMES.get(st[tag], st[tag])}: {ctxs[tag].lib.last_error(ctxs[tag].handle)}"
        if isinstance(st.get("O"), int):
            assert row.name in ORACLE_REFUSED, (row.name, s, st["O"], ctxs["O"].lib.last_error(ctxs["O"].handle))
            oracle_refused = True
            del ctxs["O"]
        if "O" in ctxs:
            e.dt = float(st["O"].dt)
        if s < STEPS_BEFORE:
            continue
        # ---- A == B, bit for bit
        a, b = ctxs["A"], ctxs["B"]
        assert a.n == b.n and stats_bits(st["A"]) == stats_bits(st["B"]), (s, stats_bits(st["A"]), stats_bits(st["B"]))
        fa, fb = all_fields(a), all_fields(b)
        try:
            same_fields(fa, fb)
        except AssertionError as err:
            k = str(err).split("\n")[0]
            bad = [(f, int((np.asarray(fa[f]).reshape(len(fa[f]), -1) != np.asarray(fb[f]).reshape(len(fb[f]), -1)).any(axis=1).sum()))
                   for f in fa if not isinstance(fa[f], int) and not isinstance(fb[f], int) and fa[f].shape == fb[f].shape
                   and not np.array_equal(fa[f].view(np.uint8), fb[f].view(np.uint8))]
            raise AssertionError(f"[{row.name}] step {s}: A != B in {k}; differing particles per field: {bad}") from None
        if s == STEPS - 1:
            (ao, ai), (bo, bi) = a.download_neighbors(), b.download_neighbors()
            assert np.array_equal(ao, bo) and np.array_equal(ai, bi), s
        if row.classes:
            for tag, c in ctxs.items():
                cls = c.download("particle_size_class")
                ref = e.classes_after[tag]
                assert np.array_equal(cls, ref), f"[{row.name}] step {s}: {tag} lost the classes sph_classify wrote for {int((cls != ref).sum())} of {len(ref)} particles"
        # ---- A ~ O
        if "O" in ctxs:
            o = ctxs["O"]
            assert a.n == o.n, s
            for f in ALL_FIELDS:
                err = rel_err(fa[f], o.download(f))
                assert err < TOL.get(f, REL_TOL_FIELDS), f"[{row.name}] step {s}: {f} against the oracle: {err:.3g}"
    assert oracle_refused == (row.name in ORACLE_REFUSED), "ORACLE_REFUSED holds a row the oracle runs"
    if row.control and profile:
        pa, pb = ctxs["A"].profile_get(), ctxs["B"].profile_get()
        assert launches(pa, "inc_reorder") >= STEPS - 2, pa     # queued ahead, as a merge ...
        assert launches(pa, "sort_scatter") <= 4, pa            # ... and adopted: the first build of the run, and nothing else
        assert "inc_reorder" not in pb, pb
    for c in ctxs.values():
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_call_sequence(lab_lib, oracle_lib, monkeypatch, row):
    run_row(row, lab_lib, lab_lib, oracle_lib, monkeypatch)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_the_oracle_runs_the_row(oracle_lib, monkeypatch, row):
    """No GPU: the oracle in all three places.  Every call of the row is one the oracle takes (or skips: it has no device, profiler,
    renderer or candidate export), its own assertions about the scene hold -- classes on both sides of the thresholds, transfers that
    move something -- and ORACLE_REFUSED names exactly the rows it refuses."""
    run_row(row, oracle_lib, oracle_lib, oracle_lib, monkeypatch, device=False)
