"""Level fields nobody has written are not moved: after sph_upload both halves of `level_estimation` and `level_old` hold the upload's
constants (FluidInterior's NaN pattern, 0) in every slot, a permutation of them is a no-op, and the reorders skip the two loads and
stores (sph_ctx::lvl_pristine) until something may write another value -- a step with a level estimation, an upload or an edit of
either field, an adaptivity entry point.  Against SPH_LEVEL_MOVE_ALWAYS=1 (every reorder moves them, as before): two contexts of one
process side by side, every per-particle download equal bit for bit after every step."""
from pathlib import Path

import numpy as np
import pytest

from adaptive_sph_amd import adaptivity as A, ffi, scene as sc
from adaptive_sph_amd.workloads import dam_break_params

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
FIELDS = ("mass", "position", "velocity", "density", "pressure", "h2", "h2_next", "level_estimation", "level_old", "particle_size_class")
LEVEL = dict(level_estimation_method="EmptyAngle", maximum_surface_distance=0.2, particle_radius_fine=0.004, particle_radius_base=0.02)
INTERIOR = 0x7fc00000   # LevelEstimationState::FluidInterior as the upload writes it
D = 1 / 64


def make_pair(lab_lib, monkeypatch, cap_factor=1):
    scn = sc.dam_break_small(64, 48, D)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    out = []
    for form in ("skip", "move"):   # (the switches are read at sph_create)
        if form == "move":
            monkeypatch.setenv("SPH_LEVEL_MOVE_ALWAYS", "1")
        g = ffi.Context(lab_lib, cap_factor * len(mass), planes)
        if form == "move":
            monkeypatch.delenv("SPH_LEVEL_MOVE_ALWAYS")
        g.upload(mass, pos, vel)
        out.append(g)
    return out[0], out[1], len(mass)


def bits(x):
    return x.view(np.uint32) if x.dtype == np.float32 else x


def step_and_compare(a, b, p, s):
    sa, sb = a.step(p), b.step(p)
    assert (np.float32(sa.dt).view(np.uint32).item(), int(sa.div_solver.iters), int(sa.density_solver.iters)) == \
           (np.float32(sb.dt).view(np.uint32).item(), int(sb.div_solver.iters), int(sb.density_solver.iters)), s
    assert a.n == b.n, s
    for f in FIELDS:
        assert np.array_equal(bits(a.download(f)), bits(b.download(f))), (s, f)
    return float(sa.dt)


def constants_in_host_order(c, n):
    assert np.array_equal(c.download("level_estimation").view(np.uint32), np.full(n, INTERIOR, np.uint32))
    assert np.array_equal(c.download("level_old").view(np.uint32), np.zeros(n, np.uint32))


def test_level_estimation_switched_on_after_steps_without_it(lab_lib, monkeypatch):
    a, b, n = make_pair(lab_lib, monkeypatch)
    p_off, p_on = dam_break_params().to_ffi(), dam_break_params(**LEVEL).to_ffi()
    for s in range(6):
        step_and_compare(a, b, p_off, s)
        for c in (a, b):
            constants_in_host_order(c, n)   # a download while the fields are not moved: what it returned before
    for s in range(6, 12):
        step_and_compare(a, b, p_on, s)
    lv = a.download("level_estimation")
    assert np.isfinite(lv).any() and len(np.unique(a.download("level_old"))) > 1   # the estimation did write both fields
    a.close()
    b.close()


def test_uploaded_level_old_travels_with_its_particles(lab_lib, monkeypatch):
    a, b, n = make_pair(lab_lib, monkeypatch)
    p = dam_break_params().to_ffi()
    ident = np.arange(n, dtype=np.float32) + 1.0
    for s in range(8):
        step_and_compare(a, b, p, s)
        if s == 3:
            for c in (a, b):
                c.upload_field("level_old", ident)
        if s >= 4:   # behind the reorders of the following steps every particle still holds its own value, in both contexts
            for c in (a, b):
                assert np.array_equal(c.download("level_old"), ident), s
                assert np.array_equal(c.download("level_estimation").view(np.uint32), np.full(n, INTERIOR, np.uint32)), s
    moved = a.download("position") - sc.init_particles(sc.dam_break_small(64, 48, D))[0]
    assert np.abs(moved).max() > 0   # (the column did start to move: the reorders were not identities by construction)
    a.close()
    b.close()


def test_split_in_the_middle(lab_lib, monkeypatch):
    """Three steps, then one adaptive step: every seventh particle marked TooLarge splits into three children, the vector is regathered
    with more particles than before -- from there on the level fields move with them."""
    a, b, n = make_pair(lab_lib, monkeypatch, cap_factor=2)
    # target mass at the surface (level 0) = pi r_fine^2 rho_0 = a third of a particle's mass: three children
    P = dam_break_params(particle_radius_fine=float(D * np.sqrt(1.0 / (3.0 * np.pi))), particle_radius_base=4 * D, maximum_surface_distance=0.2)
    p = P.to_ffi()
    sp = A.SplitPatterns.load_from_file(REPO / "tests" / "golden" / "split-patterns.yaml")
    dt = 0.0
    for s in range(3):
        dt = step_and_compare(a, b, p, s)
    cls = np.full(n, A.OPTIMAL, np.uint8)
    cls[::7] = A.TOO_LARGE
    ap = A.adapt_params(P, dt)
    for c in (a, b):
        constants_in_host_order(c, n)
        c.set_split_patterns(sp.patterns)
        c.upload_field("particle_size_class", cls)
        c.upload_field("level_estimation", np.zeros(n, np.float32))
        c.split_particles(p, ap)
    assert a.n == b.n > n, (a.n, b.n, n)
    for f in FIELDS:
        if f not in ("density", "pressure"):   # (per-step outputs: the next step writes them)
            assert np.array_equal(bits(a.download(f)), bits(b.download(f))), f
    for s in range(3, 7):
        step_and_compare(a, b, p, s)
    a.close()
    b.close()
