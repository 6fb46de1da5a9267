"""The candidate export on the device (include/sph_candidates.h): sph_download_partner_candidates against the host filter
adaptivity.partner_candidates_reference applied to the device's own full lists and fields, entry by entry; the adaptive driver in
export="candidates" mode against export="lists" (same partner arrays after every pass, bit-identical states); sph_sum_mass."""
from pathlib import Path

import numpy as np
import pytest

from adaptive_sph_amd import adaptivity as A, ffi, scene as sc
from adaptive_sph_amd.simulation import init_fluid_sim
from adaptive_sph_amd.workloads import WORKLOADS, dam_break_params, default_params

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
PATTERNS = REPO / "tests" / "golden" / "split-patterns.yaml"
RADII = dict(particle_radius_fine=0.012, particle_radius_base=0.05, maximum_surface_distance=0.3)   # test_share_and_merge_match_the_oracle
ALLOW = ["allow_share_with_optimal_particle", "allow_share_with_too_small_particle", "allow_merge_with_optimal_particle",
         "allow_merge_on_size_difference"]
DECISION_FIELDS = ("particle_size_class", "mass", "level_estimation", "position", "h2")


def default_scene():
    scn = sc.SceneConfig.from_yaml(str(REPO / "tests" / "golden" / "default-scene.yaml"))
    pos, mass, vel = sc.init_particles(scn)
    return pos, mass, vel, sc.boundary_planes(scn.boundary)


def stepped(lib, P, steps=2, policy=None, cap=70000, scene=None):
    pos, mass, vel, planes = scene if scene is not None else default_scene()
    g = ffi.Context(lib, cap, planes)
    if policy is not None:
        g.set_math_policy(policy)
    g.upload(mass, pos, vel)
    p = P.to_ffi()
    for _ in range(steps):
        st = g.step(p)
    return g, p, float(st.dt)


def all_fields(g):
    """Every field sph_download serves in the context's current state: name -> array (or the refusal's status)."""
    out = {}
    for name in ffi.FIELDS:
        try:
            out[name] = g.download(name).copy()
        except ffi.SphError as e:
            out[name] = e.status
    return out


def same_fields(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], int) or isinstance(b[k], int):
            assert isinstance(a[k], int) and isinstance(b[k], int) and a[k] == b[k], k
        else:
            assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def cut_counts(kind, f, off, idx, P):
    """(entries of donor rows without the self entries, entries the class test leaves, entries both tests leave) by the host filter."""
    cls = f["particle_size_class"]
    rows = np.repeat(np.arange(len(cls)), np.diff(off.astype(np.int64)))
    donor = cls[rows] == (A.LARGE if kind == "share" else A.TOO_SMALL)
    entries = int((donor & (rows != idx)).sum())
    wide = P.replace(max_share_distance=1e6, max_merge_distance=1e6)
    n_class = len(A.partner_candidates_reference(kind, cls, f["mass"], f["position"], f["h2"], off, idx, wide)[1])
    n_both = len(A.partner_candidates_reference(kind, cls, f["mass"], f["position"], f["h2"], off, idx, P)[1])
    return entries, n_class, n_both


def check_index_sets(g, P, dt, label, first_export_is_candidates=False):
    """Both kinds on the context's current state; returns per kind (donor-row entries, after class, after both)."""
    p, ap = P.to_ffi(), A.adapt_params(P, dt)
    early = {k: g.download_partner_candidates(k, p, ap) for k in ("share", "merge")} if first_export_is_candidates else {}
    off, idx = g.download_neighbors()
    f = {k: g.download(k) for k in DECISION_FIELDS}
    host = ffi.HostBuffers()
    out = {}
    for kind in ("share", "merge"):
        roff, ridx = A.partner_candidates_reference(kind, f["particle_size_class"], f["mass"], f["position"], f["h2"], off, idx, P)
        exports = [g.download_partner_candidates(kind, p, ap), g.download_partner_candidates(kind, p, ap, host)]
        if kind in early:
            exports.append(early[kind])   # (built by the candidate call itself, before any sph_download_neighbors of this step)
        for coff, cidx in exports:
            assert coff.dtype == np.uint32 and cidx.dtype == np.uint32
            assert np.array_equal(coff, roff), (label, kind)
            assert np.array_equal(cidx, ridx), (label, kind)
        entries, n_class, n_both = cut_counts(kind, f, off, idx, P)
        print(f"{label} {kind}: n={g.n} list entries={len(idx)} donor-row entries={entries} after class={n_class} candidates={n_both}")
        assert entries > 0, (label, kind, "no donors")
        assert n_both == len(ridx) < entries, (label, kind)
        out[kind] = (entries, n_class, n_both)
    return out


def test_index_sets_on_the_default_scene(product_lib):
    """FAST and EXACT policy, the step's lists and the extended lists of the advected positions (level_estimation_after_advection),
    the four allow_* flags off and on.  Over the cases each test must have removed entries and each must have kept some."""
    cut_class = cut_dist = kept = 0
    for policy in ("fast", "exact"):
        for after in (False, True):
            P0 = default_params(level_estimation_after_advection=after, **RADII)
            g, p, dt = stepped(product_lib, P0, policy=policy)
            g.classify(p)
            for k, allow in enumerate((False, True)):
                P = P0.replace(**{a: allow for a in ALLOW})
                res = check_index_sets(g, P, dt, f"default[{policy},after={after},allow={allow}]", first_export_is_candidates=(k == 0))
                for entries, n_class, n_both in res.values():
                    cut_class += entries - n_class
                    cut_dist += n_class - n_both
                    kept += n_both
            g.step(p)   # neither export poisoned anything
            g.close()
    assert cut_class > 0 and cut_dist > 0 and kept > 0, (cut_class, cut_dist, kept)


def test_index_sets_on_the_1m_contact_scene(product_lib):
    """dam_break_1m_adaptive_contact: 942 080 fine + 58 880 coarse particles (4:1 radii) in contact, EmptyAngle level estimation,
    sizing radii = the two blocks' particle radii (as test_config4_ratio_stress_4m_adaptive_steps sets them for its scene)."""
    scene_f, _, _ = WORKLOADS["dam_break_1m_adaptive_contact"]
    scn = scene_f()
    pos, mass, vel = sc.init_particles(scn)
    r_fine = float(np.sqrt(np.float32(0.0009765625) ** 2 * 0.93 / np.pi))
    P = dam_break_params(level_estimation_method="EmptyAngle", particle_radius_fine=r_fine, particle_radius_base=4 * r_fine,
                         maximum_surface_distance=0.3, max_iters=3)
    g, p, dt = stepped(product_lib, P, cap=len(mass), scene=(pos, mass, vel, sc.boundary_planes(scn.boundary, P.init_boundary_handler)))
    assert g.n == 1000960
    g.classify(p)
    res = check_index_sets(g, P, dt, "contact_1m", first_export_is_candidates=True)
    assert sum(n_both for _, _, n_both in res.values()) > 0
    g.step(p)


def test_merge_candidates_after_a_share(product_lib):
    """single_step_adaptivity's order: the merge search runs after share_particles on the step's unchanged lists.  Lists downloaded
    BEFORE the share, fields AFTER it; one context exports the lists to the host first, its twin only ever asks for candidates."""
    P = default_params(**RADII)
    a, p, dt = stepped(product_lib, P)
    b, _, _ = stepped(product_lib, P)
    ap = A.adapt_params(P, dt)
    a.classify(p)
    b.classify(p)
    off, idx = a.download_neighbors()
    f0 = {k: a.download(k) for k in DECISION_FIELDS}
    soff, sidx = b.download_partner_candidates("share", p, ap)          # (b builds the device CSR here)
    mp, mc = A._find_partners("share", *[f0[k] for k in DECISION_FIELDS], off, idx, P, dt)
    mp_b, mc_b = A._find_partners("share", *[f0[k] for k in DECISION_FIELDS], soff, sidx, P, dt)
    assert np.array_equal(mp, mp_b) and np.array_equal(mc, mc_b) and mc.sum() > 0
    for c in (a, b):
        c.share_particles(p, ap, mp, mc)
        c.classify(p)
    with pytest.raises(ffi.SphError):
        a.download_neighbors()                                           # (unchanged: the full export is refused after a share)
    f1 = {k: a.download(k) for k in DECISION_FIELDS}
    moved = np.nonzero((f1["position"] != f0["position"]).any(axis=1) | (f1["mass"] != f0["mass"]))[0]
    assert len(moved) > 0
    rows = np.repeat(np.arange(a.n), np.diff(off.astype(np.int64)))
    in_merge_donor_row = (f1["particle_size_class"][rows] == A.TOO_SMALL) & np.isin(idx, moved)
    assert in_merge_donor_row.any()                                      # the share moved somebody a merge donor looks at
    roff, ridx = A.partner_candidates_reference("merge", f1["particle_size_class"], f1["mass"], f1["position"], f1["h2"], off, idx, P)
    stale = A.partner_candidates_reference("merge", f0["particle_size_class"], f0["mass"], f0["position"], f0["h2"], off, idx, P)
    print(f"after a share: {int(mc.sum())} shares moved {len(moved)} particles; merge candidates {len(ridx)} (from the pre-share fields: {len(stale[1])})")
    for c in (a, b):
        coff, cidx = c.download_partner_candidates("merge", p, ap)
        assert np.array_equal(coff, roff) and np.array_equal(cidx, ridx)
        c.step(p)


class _Capture:
    """Wraps ctx.share_particles / ctx.merge_particles of one context: keeps a copy of the partner arrays of every pass."""

    def __init__(self, ctx):
        self.passes = []
        for name in ("share_particles", "merge_particles"):
            inner = getattr(ctx, name)

            def wrapped(p, ap, mp, mc, _inner=inner, _name=name):
                self.passes.append((_name, np.array(mp, copy=True), np.array(mc, copy=True)))
                return _inner(p, ap, mp, mc)
            setattr(ctx, name, wrapped)


def run_both_modes(product_lib, P, scn, steps, cap):
    sp = A.SplitPatterns.load_from_file(PATTERNS)
    sims = {m: init_fluid_sim(P, scn, lib=product_lib, split_patterns=sp, n_capacity=cap, adaptivity_export=m) for m in ("lists", "candidates")}
    caps = {m: _Capture(s.ctx) for m, s in sims.items()}
    events = {m: {"shares": 0, "merges": 0, "splits": 0} for m in sims}
    exported = {m: 0 for m in sims}
    for s in range(steps):
        for m, sim in sims.items():
            dt = sim.single_step_without_adaptivity(P)
            info = sim.single_step_adaptivity(P, dt)
            assert info["export"] == m
            exported[m] += info["exported_indices"]
            for k in events[m]:
                events[m][k] += info[k]
        la, ca = caps["lists"].passes, caps["candidates"].passes
        assert len(la) == len(ca) > 0
        for (n1, mp1, mc1), (n2, mp2, mc2) in zip(la, ca):
            assert n1 == n2 and np.array_equal(mp1, mp2) and np.array_equal(mc1, mc2), (s, n1)
        la.clear()
        ca.clear()
        assert events["lists"] == events["candidates"], (s, events)
        assert sims["lists"].num_fluid_particles() == sims["candidates"].num_fluid_particles()
    return sims, events["lists"], exported


def test_whole_driver_on_the_default_config(product_lib):
    """BASELINE configs[0] (default-config.yaml, as test_adaptive_run_of_the_default_config), 12 calls of single_step per mode from the
    same upload: the partner arrays of every pass, the event counts, n and every downloadable field at the end are identical, and so
    is the state after one more plain step.  Shares, merges and splits must all occur over the run."""
    scn = sc.SceneConfig.from_yaml(str(REPO / "tests" / "golden" / "default-scene.yaml"))
    P = default_params()
    sims, events, exported = run_both_modes(product_lib, P, scn, 12, 120000)
    print(f"configs[0]: events {events}, exported indices over 12 steps {exported}")
    assert all(v > 0 for v in events.values()), events
    same_fields(all_fields(sims["lists"].ctx), all_fields(sims["candidates"].ctx))
    for sim in sims.values():
        sim.single_step_without_adaptivity(P)
    same_fields(all_fields(sims["lists"].ctx), all_fields(sims["candidates"].ctx))
    for sim in sims.values():
        sim.close()


def test_config4_at_full_size_in_both_modes(product_lib):
    """configs[4]'s scene and radii (test_config4_ratio_stress_4m_adaptive_steps), one odd (split) and one even (merge) adaptive step
    per mode: identical partner arrays and counts, and the candidates mode exports fewer indices."""
    scene_f, params_f, _ = WORKLOADS["ratio_stress_4m"]
    r_fine = float(np.sqrt(np.float32(0.0004385) ** 2 * 0.93 / np.pi))
    P = params_f(level_estimation_method="EmptyAngle", merging=True, sharing=True, splitting=True, particle_radius_fine=r_fine,
                 particle_radius_base=50 * r_fine, maximum_surface_distance=0.3)
    sims, events, exported = run_both_modes(product_lib, P, scene_f(), 2, 6000000)
    print(f"configs[4]: events {events}, exported indices over 2 steps: lists {exported['lists']}, candidates {exported['candidates']}")
    assert events["merges"] > 1000, events
    assert 0 < exported["candidates"] < exported["lists"], exported
    for name in ("mass", "position", "velocity", "h2", "level_estimation", "particle_size_class"):
        a, b = sims["lists"].ctx.download(name), sims["candidates"].ctx.download(name)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    for sim in sims.values():
        sim.close()


@pytest.mark.parametrize("workload", ["dam_break_1m_adaptive_contact", "ratio_stress_4m"])
def test_sum_mass_against_numpy(product_lib, workload):
    """|device - numpy| <= 2 n 2^-53 numpy: every f64 addition of positive terms errs by at most 2^-53 relative, so any summation
    order is within n 2^-53 of the exact sum and two orders within twice that (3.7e-10 absolute at 1 M, 1.3e-9 at 4 M for these
    scenes).  Seen on an MI355X: a difference of 0 in both scenes (1.6710937628522515 and 1.4198985412626826 from both sides)."""
    scn = WORKLOADS[workload][0]()
    pos, mass, vel = sc.init_particles(scn)
    g = ffi.Context(product_lib, len(mass), sc.boundary_planes(scn.boundary))
    g.upload(mass, pos, vel)
    n = g.n
    assert n == len(mass) >= 1000000
    d1, d2 = g.sum_mass(), g.sum_mass()
    assert np.float64(d1).tobytes() == np.float64(d2).tobytes()
    ref = float(np.sum(g.download("mass"), dtype=np.float64))
    print(f"sum_mass {workload}: n={n} device={d1!r} numpy={ref!r} |diff|={abs(d1 - ref):.3e} bound={2 * n * 2.0 ** -53 * ref:.3e}")
    assert abs(d1 - ref) <= 2 * n * 2.0 ** -53 * ref


def test_sum_mass_across_a_share_and_the_exports_change_nothing(product_lib):
    P = default_params(**RADII)
    g, p, dt = stepped(product_lib, P)
    twin, _, _ = stepped(product_lib, P)
    ap = A.adapt_params(P, dt)
    g.classify(p)
    twin.classify(p)
    before = all_fields(g)
    m0 = g.sum_mass()
    assert np.float64(m0).tobytes() == np.float64(g.sum_mass()).tobytes()
    assert abs(m0 - float(np.sum(before["mass"], dtype=np.float64))) <= 2 * g.n * 2.0 ** -53 * m0
    cands = {k: g.download_partner_candidates(k, p, ap) for k in ("share", "merge")}
    same_fields(before, all_fields(g))                     # neither call changed anything sph_download serves
    g.download_neighbors()                                 # (the full export still works beside the filtered one)
    f = [before[k] for k in DECISION_FIELDS]
    mp, mc = A._find_partners("share", *f, *cands["share"], P, dt)
    assert mc.sum() > 0
    g.share_particles(p, ap, mp, mc)
    twin.share_particles(p, ap, mp, mc)
    m1 = g.sum_mass()
    print(f"sum_mass before / after {int(mc.sum())} shares: {m0!r} / {m1!r}, relative {abs(m1 - m0) / m0:.3e}")
    assert abs(m1 - m0) <= 1e-6 * m0                       # f32 transfers
    g.download_partner_candidates("merge", p, ap)
    g.step(p)
    twin.step(p)                                           # the twin never exported anything
    same_fields(all_fields(g), all_fields(twin))


def test_refusals(product_lib):
    from adaptive_sph_amd import distributed as D
    P = default_params(**RADII)
    pos, mass, vel, planes = default_scene()
    p = P.to_ffi()
    g = ffi.Context(product_lib, 70000, planes)
    g.upload(mass, pos, vel)
    ap = A.adapt_params(P, 1e-3)

    def refused(status, f, *a):
        with pytest.raises(ffi.SphError) as e:
            f(*a)
        assert e.value.status == status, e.value

    refused(1, g.download_partner_candidates, "share", p, ap)            # before any step
    dt = float(g.step(p).dt)
    ap = A.adapt_params(P, dt)
    g.classify(p)
    refused(1, g.download_partner_candidates, 2, p, ap)                  # kind
    refused(1, g.download_partner_candidates, "merge", None, ap)         # null params
    off, idx = g.download_partner_candidates("merge", p, ap)
    assert len(idx) > 1
    import ctypes as C
    short = np.empty(len(idx) - 1, np.uint32)
    total = C.c_uint64(0)
    rc = product_lib.download_partner_candidates(g.handle, 1, C.byref(p), C.byref(ap), None, short.ctypes.data, short.size, C.byref(total))
    assert rc == 1 and int(total.value) == len(idx)                      # capacity one short: status 1, n_indices set
    rc = product_lib.download_partner_candidates(g.handle, 1, C.byref(p), C.byref(ap), None, None, 0, C.byref(total))
    assert rc == 0 and int(total.value) == len(idx)                      # the sizing call
    f = [g.download(k) for k in DECISION_FIELDS]
    mp, mc = A._find_partners("merge", *f, off, idx, P, dt)
    assert mc.sum() > 0
    g.merge_particles(p, ap, mp, mc)
    refused(1, g.download_partner_candidates, "merge", p, ap)            # after merge_particles
    g.step(p)
    g.classify(p)
    g.download_partner_candidates("merge", p, ap)
    g.upload(mass, pos, vel)
    refused(1, g.download_partner_candidates, "merge", p, ap)            # after upload
    g.step(p)
    # a slab context (member of a loopback group): both calls are unsupported, and the group steps afterwards
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 2)
    ffi.group_step(grp, p)
    refused(30, grp[0].download_partner_candidates, "share", p, ap)
    refused(30, grp[0].sum_mass)
    ffi.group_step(grp, p)
