"""The compact partner problem's contract on the host (no GPU): adaptivity.partner_problem_reference -- the candidate rows restricted to
their participants and renumbered in ascending host index -- hands `_find_partners` a problem of size K whose decisions, expanded by
adaptivity.expand_partner_decisions, are the decisions on the full lists (include/sph_partner_problem.h).  State: that of
tests/test_candidates_host.py (the CPU oracle, default scene with 1 035 particles, two steps, the same radii)."""
import re
from pathlib import Path

import numpy as np
import pytest

from adaptive_sph_amd import adaptivity as A, ffi, scene as sc
from adaptive_sph_amd.workloads import default_params

REPO = Path(__file__).resolve().parent.parent
RADII = dict(particle_radius_fine=0.012, particle_radius_base=0.05, maximum_surface_distance=0.3)
ALLOW = ["allow_share_with_optimal_particle", "allow_share_with_too_small_particle", "allow_merge_with_optimal_particle",
         "allow_merge_on_size_difference"]
CASES = [{}] + [{a: True} for a in ALLOW] + [{"max_share_distance": d, "max_merge_distance": d} for d in (0.5, 2.0)]
FIELDS = ("particle_size_class", "mass", "level_estimation", "position", "h2")


@pytest.fixture(scope="module")
def state(oracle_lib):
    scn = sc.SceneConfig.from_yaml(str(REPO / "tests" / "golden" / "default-scene.yaml"))
    pos, mass, vel = sc.init_particles(scn)
    o = ffi.Context(oracle_lib, 70000, sc.boundary_planes(scn.boundary))
    o.upload(mass, pos, vel)
    P = default_params(**RADII)
    p = P.to_ffi()
    for _ in range(2):
        st = o.step(p)
    o.classify(p)
    f = {k: o.download(k) for k in FIELDS}
    off, idx = o.download_neighbors()
    return o, P, float(st.dt), f, off, idx


def _problem(kind, P, f, off, idx):
    return A.partner_problem_reference(kind, *[f[k] for k in FIELDS], off, idx, P)


@pytest.mark.parametrize("kind", ["share", "merge"])
@pytest.mark.parametrize("over", CASES, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()) or "default")
def test_decisions_on_the_compact_problem_are_the_decisions_on_the_full_lists(state, kind, over):
    _, P, dt, f, off, idx = state
    P = P.replace(**over)
    n = len(f["mass"])
    full = A._find_partners(kind, *[f[k] for k in FIELDS], off, idx, P, dt)
    ids, *fields_c, off_c, idx_c = _problem(kind, P, f, off, idx)
    K = len(ids)
    assert all(len(a) == K for a in fields_c) and len(off_c) == K + 1 and int(off_c[-1]) == len(idx_c)
    mp_c, mc_c = A._find_partners(kind, *fields_c, off_c, idx_c, P, dt)
    assert len(mp_c) == len(mc_c) == K
    A.validate_partners(kind, fields_c[0], mp_c, mc_c, off_c, idx_c)
    mp, mc = A.expand_partner_decisions(n, ids, mp_c, mc_c)
    assert mp.dtype == np.uint32 and mc.dtype == np.uint16
    assert np.array_equal(full[0], mp) and np.array_equal(full[1], mc)
    if not over:
        assert int(full[1].sum()) > 0     # (the default case decides something: the equality above is not one of two empty answers)


@pytest.mark.parametrize("kind", ["share", "merge"])
def test_structure_of_the_compact_problem(state, kind):
    _, P, dt, f, off, idx = state
    n = len(f["mass"])
    coff, cidx = A.partner_candidates_reference(kind, f["particle_size_class"], f["mass"], f["position"], f["h2"], off, idx, P)
    ids, cls_c, mass_c, lvl_c, pos_c, h2_c, off_c, idx_c = _problem(kind, P, f, off, idx)
    K = len(ids)
    assert ids.dtype == np.uint32 and off_c.dtype == np.uint32 and idx_c.dtype == np.uint32
    assert np.all(np.diff(ids.astype(np.int64)) > 0) and (K == 0 or int(ids[-1]) < n)
    for name, got in zip(FIELDS, (cls_c, mass_c, lvl_c, pos_c, h2_c)):
        assert got.dtype == f[name].dtype and np.array_equal(got.view(np.uint8), np.ascontiguousarray(f[name][ids]).view(np.uint8)), name
    assert pos_c.shape == (K, 2)
    assert len(idx_c) == len(cidx) and (len(idx_c) == 0 or int(idx_c.max()) < K)
    for c in range(K):       # every compact row maps through ids to the candidate row of that particle
        i = int(ids[c])
        assert np.array_equal(ids[idx_c[off_c[c]:off_c[c + 1]]], cidx[coff[i]:coff[i + 1]]), (c, i)
    rest = np.setdiff1d(np.arange(n), ids)
    assert len(rest) == n - K
    assert np.all(coff[rest + 1] == coff[rest])          # a non-participant's candidate row is empty
    assert not np.isin(cidx, rest).any()                 # ... and it occurs in no row
    assert K <= 2 * len(idx_c)


def test_the_share_problem_of_the_default_state_is_small(state):
    """profiles/r8_candidates.md records 77 share candidates on this state: at most 77 entries plus 77 owning rows take part."""
    _, P, dt, f, off, idx = state
    n = len(f["mass"])
    ids = _problem("share", P, f, off, idx)[0]
    print(f"share problem of the default state: K={len(ids)} of n={n}")
    assert 0 < len(ids) <= 154 < n


def test_expand_leaves_the_sentinels_alone():
    ids = np.array([2, 5, 9], np.uint32)
    mp_c = np.array([A.MERGE_PARTNER_DELETE, 0, A.MERGE_PARTNER_AVAILABLE], np.uint32)
    mc_c = np.array([1, 0, 0], np.uint16)
    mp, mc = A.expand_partner_decisions(11, ids, mp_c, mc_c)
    want = np.full(11, A.MERGE_PARTNER_AVAILABLE, np.uint32)
    want[2], want[5] = A.MERGE_PARTNER_DELETE, 2
    assert np.array_equal(mp, want) and mc.tolist() == [0, 0, 1] + [0] * 8
    mp, mc = A.expand_partner_decisions(4, np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint16))
    assert np.all(mp == A.MERGE_PARTNER_AVAILABLE) and not mc.any()


def test_driver_modes():
    class _Ctx:
        n = 0
    assert A.AdaptivityDriver.EXPORTS == ("lists", "candidates", "compact")
    d = A.AdaptivityDriver(_Ctx(), export="compact")
    assert d.export == "compact"
    with pytest.raises(ValueError):
        A.AdaptivityDriver(_Ctx(), export="everything")
    with pytest.raises(ValueError):
        d.single_step_adaptivity(default_params(), 1e-3, 2, lists=(np.zeros(1, np.uint32), np.zeros(0, np.uint32)))
    h = ffi.HostBuffers()
    h.reserve(1000, export="compact")
    assert h.capacity("csr:indices", np.uint32) == 0 and h.capacity("cand:indices", np.uint32) == 0
    assert h.capacity("prob:offsets", np.uint32) >= 1001 and h.capacity("prob:ids", np.uint32) >= 1000
    for name in FIELDS:
        assert h.capacity("prob:" + name, ffi.FIELDS[name][1]) >= 1000 * ffi.FIELDS[name][2], name
    assert h.capacity("prob:indices", np.uint32) > 0


def test_symbols_header_and_the_oracles_refusal(state, product_lib, oracle_lib):
    header = (REPO / "include" / "sph_partner_problem.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sph_[a-z_0-9]+)\s*\(", header)))
    assert declared == sorted("sph_" + s for s in ffi.PROBLEM_SYMBOLS)
    for s in ffi.PROBLEM_SYMBOLS:
        assert hasattr(product_lib.lib, "sph_" + s), s
        assert s not in ffi.ABI_SYMBOLS and s not in ffi.CANDIDATE_SYMBOLS
        assert getattr(product_lib, s) is not None and getattr(oracle_lib, s) is None
    o, P, dt = state[0], state[1], state[2]
    p, ap = P.to_ffi(), A.adapt_params(P, dt)
    none = (np.zeros(0, np.uint32), np.zeros(0, np.uint16))
    for call in (lambda: o.download_partner_problem("share", p, ap), lambda: o.download_partner_problem("merge", p, ap, ffi.HostBuffers(), want_ids=True),
                 lambda: o.share_particles_compact(p, ap, *none), lambda: o.merge_particles_compact(p, ap, *none)):
        with pytest.raises(ffi.SphError) as e:
            call()
        assert e.value.status == 30
