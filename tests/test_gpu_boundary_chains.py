"""The solve's tail on tiles -- one workgroup per U x 256 consecutive particles, everything a lane reads of its U particles requested
together (sph_sweeps.hip: k_solver_tail<TAIL, U>), one header partial per tile -- and the place launch that reads a stayer's rank off
its wave's ballot (sph_sort.hip: k_inc_place_reorder, the slab ranks' PERM form included) against the forms they replace
(SPH_BOUNDARY_CHAINS=0: one particle per lane, its loads one behind the other, one partial per 256 particles; the rank as a loop over
single flag bytes).  Two contexts of one process step side by
side; after every step: dt, both iteration counts, the grid, the cell indices, the neighbour lists, the fields and the launches of
every build scope are equal bit for bit.  (Helpers after tests/test_gpu_boundary_fused.py.)"""
import numpy as np
import pytest

from adaptive_sph_amd import ffi, scene as sc
from adaptive_sph_amd.workloads import dam_break_params
from tests.test_gpu_incremental_sort import scene_of

pytestmark = pytest.mark.gpu

STEPS = 12
FIELDS = ("position", "velocity", "density", "pressure", "cell_index")
SWITCH = "SPH_BOUNDARY_CHAINS"

# particle counts on both sides of the wave's 64, the workgroup's 256 and the tile's U x 256 (U = 2, 4): dam_break_small(w, h, spacing)
SIZES = {255: (15, 17), 256: (16, 16), 1023: (31, 33), 1024: (32, 32), 1025: (25, 41), 3080: (56, 55)}


def scene(kind):
    """An integer: a column at rest of that many particles (steps without a mover).  thrown / collide: many movers, cells entered by
    several movers, a travelling grid, a compressed front (tests/test_gpu_incremental_sort.py)."""
    if isinstance(kind, int):
        w, h = SIZES[kind]
        return sc.dam_break_small(w, h, 1 / 64), {}
    return scene_of(kind)


def grid_tuple(c):
    g = c.grid()
    return (g.cell_size, g.cells_min_x, g.cells_min_y, g.size_x, g.size_y)


def make_pair(lab_lib, monkeypatch, kind, solver, env=None, vel_edit=None):
    scn, over = scene(kind)
    pos, mass, vel = sc.init_particles(scn)
    if isinstance(kind, int):
        assert len(mass) == kind
    if vel_edit is not None:
        vel = vel_edit(vel.copy())
    P = dam_break_params(pressure_solver_method=solver, **over)
    planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    out = []
    for form in ("tiled", "serial"):   # (the switches are read at sph_create)
        if form == "serial":
            monkeypatch.setenv(SWITCH, "0")
        g = ffi.Context(lab_lib, len(mass), planes)
        if form == "serial":
            monkeypatch.delenv(SWITCH)
        g.upload(mass, pos, vel)
        g.profile_enable(1)
        out.append(g)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return out[0], out[1], P.to_ffi()


def build_launches(c):
    return {k: v[0] for k, v in c.profile_get().items() if k.startswith(("inc_", "sort_", "rs_")) or k in ("reorder", "cell_start", "header", "header_ahead")}


def stats_key(st):
    return (np.float32(st.dt).view(np.uint32).item(), int(st.div_solver.iters), int(st.density_solver.iters), int(st.density_solver.normal_count))


def step_and_compare(a, b, p, s):
    sa, sb = a.step(p), b.step(p)
    assert stats_key(sa) == stats_key(sb), s
    assert grid_tuple(a) == grid_tuple(b), s
    for f in FIELDS:
        assert np.array_equal(a.download(f), b.download(f)), (s, f)
    (oa, ia), (ob, ib) = a.download_neighbors(), b.download_neighbors()
    assert np.array_equal(oa, ob) and np.array_equal(ia, ib), s
    pa, pb = (build_launches(c) for c in (a, b))
    assert pa == pb, (s, pa, pb)


def merges(c):
    return c.profile_get().get("inc_reorder", (0, 0))[0]


CASES = [(n, "HybridDFSPH") for n in SIZES] + [(255, "IISPH"), (1025, "IISPH"), (3080, "IISPH"), (256, "OnlyDivergence"), (1025, "OnlyDivergence"),
                                                 (3080, "OnlyDivergence"), ("column", "HybridDFSPH"), ("thrown", "HybridDFSPH"), ("thrown", "OnlyDivergence"),
                                                 ("collide", "IISPH"), ("collide", "HybridDFSPH")]


@pytest.mark.parametrize("kind,solver", CASES)
def test_tiled_tail_is_the_one_particle_tail(lab_lib, monkeypatch, kind, solver):
    a, b, p = make_pair(lab_lib, monkeypatch, kind, solver)
    for s in range(STEPS):
        step_and_compare(a, b, p, s)
    pa = a.profile_get()
    print(kind, solver, a.n, {k: v[0] for k, v in pa.items() if k.startswith("inc_") or k in ("sort_scatter", "solver_tail")})
    # every build but the first of the run was queued ahead as a merge, behind the tail that classified for it
    assert merges(a) == merges(b) and merges(a) >= (STEPS - 2 if isinstance(kind, str) else 1), pa
    assert pa["solver_tail"][0] >= STEPS * (2 if solver == "HybridDFSPH" else 1), pa
    a.close()
    b.close()


def test_merge_and_radix_builds_alternate(lab_lib, monkeypatch):
    """SPH_INC_SORT=40: the merge up to n / 40 movers -- the thrown block crosses that limit back and forth."""
    a, b, p = make_pair(lab_lib, monkeypatch, "thrown", "HybridDFSPH", env=dict(SPH_INC_SORT="40"))
    for s in range(STEPS):
        step_and_compare(a, b, p, s)
    print({k: v[0] for k, v in a.profile_get().items() if k.startswith("inc_") or k == "sort_scatter"})
    a.close()
    b.close()


def test_positions_uploaded_between_steps(lab_lib, monkeypatch):
    """sph_download + sph_upload_field(position) every third step: the upload drops the header the tail's partials were reduced to and the
    build queued behind the tail -- the next step starts from k_header and a sort of its own, in both forms alike."""
    a, b, p = make_pair(lab_lib, monkeypatch, 3080, "HybridDFSPH")
    for s in range(STEPS):
        step_and_compare(a, b, p, s)
        if s % 3 == 1:
            for c in (a, b):
                x = c.download("position")
                c.upload_field("position", x + np.float32(1e-4))
    pa = a.profile_get()
    assert pa["header"][0] >= 1 + STEPS // 3, pa   # the first step's, and one after every upload
    a.close()
    b.close()


def test_infinite_velocity_raises_the_same_error(lab_lib, monkeypatch):
    """One velocity set infinite: the same error code and particle id from both forms.  (The guard that fires first is the viscosity's, in
    front of the tail, on one of the particle's neighbours: the step ends there in both forms.)"""
    def edit(v):
        v[700, 1] = np.inf
        return v
    a, b, p = make_pair(lab_lib, monkeypatch, 1025, "HybridDFSPH", vel_edit=edit)
    errs = []
    for c in (a, b):
        with pytest.raises(ffi.SphError) as e:
            for _ in range(3):
                c.step(p)
        errs.append((e.value.status, e.value.message))
    print(errs)
    assert errs[0] == errs[1], errs
    a.close()
    b.close()


def test_two_slab_ranks(lab_lib, monkeypatch):
    """A 2-rank loopback group: the tail runs over owned slots and ghosts (the `owned` flags), its header partials feed
    k_header_ahead; every rank's arrays bit for bit."""
    from adaptive_sph_amd import distributed as D
    scn, _ = scene(255)
    pos, mass, vel = sc.init_particles(scn)
    vel = vel.copy()
    vel[:, 0] = 0.8   # (pushed across the cut)
    P = dam_break_params(max_iters=6)
    planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    p = P.to_ffi()
    out = {}
    for form in ("tiled", "serial"):
        if form == "serial":
            monkeypatch.setenv(SWITCH, "0")
        grp = D.make_loopback_group(lab_lib, pos, mass, vel, planes, 2)
        if form == "serial":
            monkeypatch.delenv(SWITCH)
        for c in grp:
            c.profile_enable(1)
        its, fields = [], []
        for s in range(6):
            sts = ffi.group_step(grp, p)
            its.append(tuple(stats_key(st) for st in sts))
            fields.append([{f: c.download(f) for f in ("particle_id",) + FIELDS} for c in grp])
        out[form] = (its, fields, [c.profile_get() for c in grp])
        for c in grp:
            c.close()
    print([{k: v[0] for k, v in pr.items() if k.startswith("inc_") or k in ("solver_tail", "sort_scatter")} for pr in out["tiled"][2]])
    assert all(pr["solver_tail"][0] >= 6 for pr in out["tiled"][2]), out["tiled"][2]
    assert all(pr.get("inc_place", (0, 0))[0] >= 1 for pr in out["tiled"][2]), out["tiled"][2]   # (the ranks did merge: the PERM place ran)
    assert out["tiled"][0] == out["serial"][0]
    for s, (ra, rb) in enumerate(zip(out["tiled"][1], out["serial"][1])):
        for r, (fa, fb) in enumerate(zip(ra, rb)):
            for f in fa:
                assert np.array_equal(fa[f], fb[f]), (s, r, f)
