"""The partner search's parallel schedule on the host (no GPU): adaptivity.find_partners_frontier -- the numpy twin of
csrc/sph_partner_search.hip, DESIGN.md section 10.3 -- takes the decisions of the sequential loop `_find_partners`, array for array, on the
compact problems of tests/test_partner_problem_host.py (the CPU oracle's default scene, two steps, the same radii and CASES), on the same
scene at half block spacing (K beyond one scan tile of 2 048) and on synthetic CSRs with no scene behind them.  The twin itself asserts
the schedule's two invariants in every round: the frontier's touch sets are disjoint on unclaimed particles, and the smallest undecided
donor is in it."""
from pathlib import Path

import numpy as np
import pytest
import yaml

from adaptive_sph_amd import adaptivity as A, ffi, scene as sc
from adaptive_sph_amd.workloads import default_params
from tests.test_partner_problem_host import CASES, FIELDS, RADII

REPO = Path(__file__).resolve().parent.parent


def _oracle_state(oracle_lib, spacing_factor):
    doc = yaml.safe_load((REPO / "tests" / "golden" / "default-scene.yaml").read_text())
    for b in doc["blocks"]:
        b["spacing"] = b["spacing"] * spacing_factor
    scn = sc.SceneConfig.from_mapping(doc)
    pos, mass, vel = sc.init_particles(scn)
    o = ffi.Context(oracle_lib, 70000, sc.boundary_planes(scn.boundary))
    o.upload(mass, pos, vel)
    P = default_params(**RADII)
    p = P.to_ffi()
    for _ in range(2):
        st = o.step(p)
    o.classify(p)
    f = [o.download(k) for k in FIELDS]
    off, idx = o.download_neighbors()
    o.close()
    return P, float(st.dt), f, off, idx


@pytest.fixture(scope="module")
def state(oracle_lib):
    return _oracle_state(oracle_lib, 1.0)


@pytest.fixture(scope="module")
def half_spacing_state(oracle_lib):
    return _oracle_state(oracle_lib, 0.5)


def _both(kind, P, dt, f, off, idx):
    """The compact problem of the state, the sequential loop and the schedule on it -> (K, info); the arrays are compared here."""
    ids, *fc, off_c, idx_c = A.partner_problem_reference(kind, *f, off, idx, P)
    mp, mc = A._find_partners(kind, *fc, off_c, idx_c, P, dt)
    mp2, mc2, info = A.find_partners_frontier(kind, *fc, off_c, idx_c, P, dt)
    assert mp2.dtype == np.uint32 and mc2.dtype == np.uint16
    assert np.array_equal(mp, mp2) and np.array_equal(mc, mc2)
    A.validate_partners(kind, fc[0], mp2, mc2, off_c, idx_c)
    assert info["participants"] == len(ids) and info["candidates"] == len(idx_c)
    assert info["transfers"] == int(mc.sum()) and info["donors"] == int(np.count_nonzero(mc))
    assert info["rounds"] <= max(1, int(np.count_nonzero(np.diff(off_c.astype(np.int64))))) and info["max_frontier"] >= (1 if len(idx_c) else 0)
    return len(ids), info


@pytest.mark.parametrize("kind", ["share", "merge"])
@pytest.mark.parametrize("over", CASES, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()) or "default")
def test_the_schedule_takes_the_loops_decisions(state, kind, over):
    P, dt, f, off, idx = state
    K, info = _both(kind, P.replace(**over), dt, f, off, idx)
    print(f"{kind} {over}: K={K} {info}")
    if not over and kind == "merge":
        assert info["rounds"] > 1 and info["transfers"] > 0


def test_the_schedule_beyond_one_scan_tile(half_spacing_state):
    P, dt, f, off, idx = half_spacing_state
    assert len(f[1]) == 4176
    K, info = _both("merge", P, dt, f, off, idx)
    print(f"merge at half spacing: K={K} {info}")
    assert K > 2048 and info["rounds"] > 1 and info["transfers"] > 0
    _both("share", P, dt, f, off, idx)


def synthetic_grid(w, h, order, seed=7):
    """A jittered w x h grid with every particle TooSmall, uniform mass m, target mass 4 m and mass_base 6 m: a merge donor takes every
    neighbour that is still available.  order "grid": x-outer index order; "random": the same particles in a random permutation.
    -> (P, dt, fields, offsets, indices), rows = the particles within 1.5 spacings in ascending index."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
    pos = np.stack([gx.ravel(), gy.ravel()], 1).astype(np.float64) + rng.uniform(-0.2, 0.2, (w * h, 2))
    n = w * h
    if order == "random":
        pos = pos[rng.permutation(n)]
    pos = pos.astype(np.float32)
    d2 = ((pos[:, None, :].astype(np.float64) - pos[None, :, :]) ** 2).sum(-1)
    near = (d2 < 1.5 ** 2) & ~np.eye(n, dtype=bool)
    rows, cols = np.nonzero(near)                      # row-major: every row ascending
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum(np.bincount(rows, minlength=n))
    idx = cols.astype(np.uint32)
    m, rho0, msd = 1e-3, 1.0, 0.3
    P = default_params(particle_radius_fine=float(np.sqrt(2 * m / (np.pi * rho0))), particle_radius_base=float(np.sqrt(6 * m / (np.pi * rho0))),
                       maximum_surface_distance=msd, rest_density=rho0, sizing_function="Mass", max_merge_distance=1.0)
    f = [np.full(n, A.TOO_SMALL, np.uint8), np.full(n, m, np.float32), np.full(n, -msd / 2, np.float32), pos, np.full(n, 4.0, np.float32)]
    return P, 1e-3, f, off, idx


def test_synthetic_grids_in_both_orders():
    rounds = {}
    for order in ("grid", "random"):
        P, dt, f, off, idx = synthetic_grid(32, 32, order)
        assert abs(float(A.target_mass(f[2], P)[0]) / 4e-3 - 1) < 1e-5 and abs(float(A.mass_base(P)) / 6e-3 - 1) < 1e-5
        mp, mc = A._find_partners("merge", *f, off, idx, P, dt)
        mp2, mc2, info = A.find_partners_frontier("merge", *f, off, idx, P, dt)
        assert np.array_equal(mp, mp2) and np.array_equal(mc, mc2)
        assert info["transfers"] == int(mc.sum()) > 0
        print(f"32x32 {order}: {info}")
        assert info["row_walks"] <= 4 * len(mc)          # work follows the frontier: a sweep per round would be n * rounds / 2
        rounds[order] = info["rounds"]
    assert rounds["grid"] > 16
    assert rounds["random"] < rounds["grid"]


def test_driver_mode():
    class _Ctx:
        n = 0
    assert A.AdaptivityDriver.DEVICE_EXPORTS == ("device",) and "device" not in A.AdaptivityDriver.EXPORTS   # (the host-decided modes stay as they were)
    d = A.AdaptivityDriver(_Ctx(), export="device")
    assert d.export == "device"
    with pytest.raises(ValueError):
        d.single_step_adaptivity(default_params(), 1e-3, 2, lists=(np.zeros(1, np.uint32), np.zeros(0, np.uint32)))
    h = ffi.HostBuffers()
    h.reserve(1000, export="device")          # nothing per particle crosses the bus: nothing to reserve
    assert all(h.capacity(k, np.uint8) == 0 for k in ("csr:indices", "cand:indices", "prob:ids", "merge_partner"))
    assert A.AdaptivityDriver.INFO_BYTES == __import__("ctypes").sizeof(ffi.SphPartnerSearchInfo) == 48


def test_symbols_header_and_the_oracles_refusal(state, product_lib, oracle_lib):
    import re
    header = (REPO / "include" / "sph_partner_search.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sph_[a-z_0-9]+)\s*\(", header)))
    assert declared == sorted("sph_" + s for s in ffi.SEARCH_SYMBOLS)
    for s in ffi.SEARCH_SYMBOLS:
        assert hasattr(product_lib.lib, "sph_" + s), s
        assert s not in ffi.ABI_SYMBOLS and s not in ffi.CANDIDATE_SYMBOLS and s not in ffi.PROBLEM_SYMBOLS
        assert getattr(product_lib, s) is not None and getattr(oracle_lib, s) is None
    P, dt = state[0], state[1]
    p, ap = P.to_ffi(), A.adapt_params(P, dt)
    scn = sc.SceneConfig.from_yaml(str(REPO / "tests" / "golden" / "default-scene.yaml"))
    o = ffi.Context(oracle_lib, 2000, sc.boundary_planes(scn.boundary))
    for call in (lambda: o.find_partners_device("share", p, ap), lambda: o.download_partner_decisions(0), lambda: o.share_particles_device(p, ap),
                 lambda: o.merge_particles_device(p, ap)):
        with pytest.raises(ffi.SphError) as e:
            call()
        assert e.value.status == 30
    o.close()
