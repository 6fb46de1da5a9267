"""The partner search on the device (include/sph_partner_search.h): the decisions of sph_find_partners_device against the sequential loop
`_find_partners` run on what sph_download_partner_problem returns for the same context, for the resident driver, the wide driver and
the default mix of the two; the apply calls against the compact path (bit-identical states); the adaptive driver in export="device"
mode against export="lists" and "compact"; the refusals and the solution's lifetime."""
from pathlib import Path

import numpy as np
import pytest
import yaml

from adaptive_sph_amd import adaptivity as A, ffi, scene as sc
from adaptive_sph_amd.simulation import init_fluid_sim
from adaptive_sph_amd.workloads import default_params
from tests.test_gpu_partner_problem import ALLOW, PATTERNS, RADII, SCAN_TILE, all_fields, default_scene, same_fields, stepped

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
THRESHOLDS = (0, 1, 0xFFFFFFFF)   # the library's default; every round wide; every round resident
INFO_KEYS = ("participants", "candidates", "donors", "transfers")
NOBODY_LARGE = dict(particle_radius_fine=0.2, particle_radius_base=0.4, maximum_surface_distance=0.3)   # every target mass far above every particle's


def search_against_the_loop(g, p, P, dt, kind, label):
    """Every threshold's decisions == the loop's on the downloaded problem; -> (K, info of the default threshold)."""
    ap = A.adapt_params(P, dt)
    ids, *fc, off_c, idx_c = g.download_partner_problem(kind, p, ap, want_ids=True)
    mp, mc = A._find_partners(kind, *fc, off_c, idx_c, P, dt)
    want = {"participants": len(ids), "candidates": len(idx_c), "donors": int(np.count_nonzero(mc)), "transfers": int(mc.sum())}
    first = None
    for thr in THRESHOLDS:
        info = g.find_partners_device(kind, p, ap, thr)
        ids2, mp2, mc2 = g.download_partner_decisions(len(ids))
        print(f"{label} {kind} threshold={thr:#x}: {info}")
        assert np.array_equal(ids, ids2), (label, kind, thr)
        assert np.array_equal(mp, mp2) and np.array_equal(mc, mc2), (label, kind, thr, int(np.count_nonzero(mp != mp2)), int(np.count_nonzero(mc != mc2)))
        assert {k: info[k] for k in INFO_KEYS} == want, (label, kind, thr)
        if thr == 1:
            assert info["wide_rounds"] == info["rounds"]
        if thr == 0xFFFFFFFF:
            assert info["wide_rounds"] == 0
        if first is None:
            first = info
        assert (info["rounds"], info["max_frontier"]) == (first["rounds"], first["max_frontier"]), (label, kind, thr)   # the schedule is one
    return len(ids), first


@pytest.mark.parametrize("policy", ["fast", "exact"])
def test_decisions_are_the_loops(product_lib, policy):
    P0 = default_params(**RADII)
    g, p, dt = stepped(product_lib, P0, policy=policy)
    g.classify(p)
    before = all_fields(g)
    for allow in (False, True):
        P = P0.replace(**{a: allow for a in ALLOW})
        for kind in ("share", "merge"):
            K, info = search_against_the_loop(g, p, P, dt, kind, (policy, allow))
            assert K > 0 and info["transfers"] > 0
            if kind == "merge":
                assert info["rounds"] >= 2
    same_fields(before, all_fields(g))   # neither the search nor the downloads wrote simulation state
    g.step(p)
    g.close()


def test_decisions_beyond_one_scan_tile(product_lib):
    """The default scene at half block spacing: K of the merge search crosses the scan tile of the rank scan and of the writers' scan."""
    doc = yaml.safe_load((REPO / "tests" / "golden" / "default-scene.yaml").read_text())
    for b in doc["blocks"]:
        b["spacing"] = b["spacing"] * 0.5
    scn = sc.SceneConfig.from_mapping(doc)
    pos, mass, vel = sc.init_particles(scn)
    assert len(mass) == 4176
    P = default_params(**RADII)
    p = P.to_ffi()
    g = ffi.Context(product_lib, 70000, sc.boundary_planes(scn.boundary))
    g.upload(mass, pos, vel)
    for _ in range(2):
        dt = float(g.step(p).dt)
    g.classify(p)
    K, info = search_against_the_loop(g, p, P, dt, "merge", "half spacing")
    assert K > SCAN_TILE and info["rounds"] >= 2 and info["transfers"] > 0
    search_against_the_loop(g, p, P, dt, "share", "half spacing")
    g.close()


def test_wide_frontiers_spills_and_hand_overs(product_lib):
    """The default scene at 0.08 of its spacing (about 160 000 particles), uploaded in a RANDOM order: neighbouring donors are far apart in
    index, so thousands are ready at once -- frontiers beyond the LDS heads of the resident kernel's lists (512 frontier, 2 048 dirty /
    recheck entries: the spill to the global arrays) and far beyond the library's default wide threshold, with hand-overs between the two
    drivers while the frontier shrinks.  Reference: the compiled sequential loop (sph_host_find_partners, the loop
    of `_find_partners`) on the downloaded problem.  600 lies between the frontier's LDS head and the largest frontier."""
    doc = yaml.safe_load((REPO / "tests" / "golden" / "default-scene.yaml").read_text())
    for b in doc["blocks"]:
        b["spacing"] = b["spacing"] * 0.08
    scn = sc.SceneConfig.from_mapping(doc)
    pos, mass, vel = sc.init_particles(scn)
    order = np.random.default_rng(11).permutation(len(mass))
    P = default_params(**RADII)
    p = P.to_ffi()
    g = ffi.Context(product_lib, len(mass), sc.boundary_planes(scn.boundary))
    g.upload(mass[order], pos[order], vel[order])
    dt = float(g.step(p).dt)
    g.classify(p)
    ap = A.adapt_params(P, dt)
    ids, *fc, off_c, idx_c = g.download_partner_problem("merge", p, ap, want_ids=True)
    mp, mc = A.find_partners_native(product_lib, "merge", *fc, off_c, idx_c, P, dt)
    infos = {}
    for thr in (0, 600, 0xFFFFFFFF):
        info = infos[thr] = g.find_partners_device("merge", p, ap, thr)
        _, mp2, mc2 = g.download_partner_decisions(len(ids))
        print(f"n={len(mass)} threshold={thr:#x}: {info}")
        assert np.array_equal(mp, mp2) and np.array_equal(mc, mc2), (thr, int(np.count_nonzero(mp != mp2)), int(np.count_nonzero(mc != mc2)))
        assert info["transfers"] == int(mc.sum()) > 0 and info["donors"] == int(np.count_nonzero(mc))
        assert (info["rounds"], info["max_frontier"]) == (infos[0]["rounds"], infos[0]["max_frontier"])
    assert infos[0]["max_frontier"] >= 4096 and infos[0]["participants"] > 100000
    assert 0 < infos[600]["wide_rounds"] < infos[600]["rounds"]          # both drivers ran
    assert 0 < infos[0]["wide_rounds"] <= infos[0]["rounds"]
    assert infos[0xFFFFFFFF]["wide_rounds"] == 0
    g.merge_particles_device(p, ap)
    assert g.n < len(mass)
    g.step(p)
    g.close()


def test_apply_is_the_compact_apply(product_lib):
    """Two contexts from one upload.  A: the compact path (problem down, the loop on the host, decisions up).  B: search and apply on the
    device.  Every downloadable field is bit-identical after each stage, and the search itself writes none of them."""
    P = default_params(**RADII)
    a, p, dt = stepped(product_lib, P)
    b, _, _ = stepped(product_lib, P)
    ap = A.adapt_params(P, dt)
    n0 = a.n
    for kind in ("share", "merge"):
        a.classify(p)
        b.classify(p)
        _, *fc, off_c, idx_c = a.download_partner_problem(kind, p, ap)
        mp_c, mc_c = A._find_partners(kind, *fc, off_c, idx_c, P, dt)
        before = all_fields(b)
        info = b.find_partners_device(kind, p, ap)
        same_fields(before, all_fields(b))
        assert info["transfers"] == int(mc_c.sum()) > 0
        if kind == "share":
            a.share_particles_compact(p, ap, mp_c, mc_c)
            b.share_particles_device(p, ap)
        else:
            a.merge_particles_compact(p, ap, mp_c, mc_c)
            b.merge_particles_device(p, ap)
        assert a.n == b.n
        same_fields(all_fields(a), all_fields(b))
    assert a.n < n0     # the merge deleted particles
    a.step(p)
    b.step(p)
    same_fields(all_fields(a), all_fields(b))


def test_whole_driver_on_the_default_config(product_lib):
    """BASELINE configs[0] (default-config.yaml), 12 calls of single_step per mode from the same upload: event counts, n and every
    downloadable field at the end are identical to the lists mode's, and so is the state after one more plain step; the device mode
    moves fewer bytes down than the compact mode and none up."""
    scn = sc.SceneConfig.from_yaml(str(REPO / "tests" / "golden" / "default-scene.yaml"))
    P = default_params()
    sp = A.SplitPatterns.load_from_file(PATTERNS)
    sims = {m: init_fluid_sim(P, scn, lib=product_lib, split_patterns=sp, n_capacity=120000, adaptivity_export=m) for m in ("lists", "compact", "device")}
    events = {m: {"shares": 0, "merges": 0, "splits": 0} for m in sims}
    down = {m: 0 for m in sims}
    participants = {m: 0 for m in sims}
    rounds = 0
    for s in range(12):
        for m, sim in sims.items():
            dt = sim.single_step_without_adaptivity(P)
            info = sim.single_step_adaptivity(P, dt)
            assert info["export"] == m
            for k in events[m]:
                events[m][k] += info[k]
            down[m] += info["bytes_down"]
            participants[m] += info["participants"]
            if m == "device":
                assert info["bytes_up"] == 0 and info["exported_indices"] == 0
                assert info["bytes_down"] == 16 + 48 * len(info["passes"])      # the two mass sums and an info struct per pass
                assert info["rounds"] == max([q["search"]["rounds"] for q in info["passes"]] + [0])
                assert info["max_frontier"] == max([q["search"]["max_frontier"] for q in info["passes"]] + [0])
                rounds = max(rounds, info["rounds"])
        assert events["lists"] == events["device"] == events["compact"], (s, events)
        assert sims["lists"].num_fluid_particles() == sims["device"].num_fluid_particles()
    print(f"configs[0]: events {events['lists']}, bytes down {down}, participants {participants}, most rounds in a pass {rounds}")
    assert all(v > 0 for v in events["lists"].values()), events
    assert participants["device"] == participants["compact"] > 0
    assert down["device"] < down["compact"] < down["lists"]
    assert rounds >= 2
    same_fields(all_fields(sims["lists"].ctx), all_fields(sims["device"].ctx))
    for sim in sims.values():
        sim.single_step_without_adaptivity(P)
    same_fields(all_fields(sims["lists"].ctx), all_fields(sims["device"].ctx))
    for sim in sims.values():
        sim.close()


def test_refusals_and_lifetime(product_lib):
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

    def fresh_step():
        nonlocal ap
        ap = A.adapt_params(P, float(g.step(p).dt))
        g.classify(p)

    refused(1, g.find_partners_device, "share", p, ap)                   # before any step: no lists
    refused(1, g.share_particles_device, p, ap)                          # no solution
    fresh_step()
    # K == 0: with radii that classify nobody Large no donor has a candidate -- an all-zero info, and the apply is that of all-AVAILABLE arrays
    p_none = default_params(**NOBODY_LARGE).to_ffi()
    g.classify(p_none)
    assert not (g.download("particle_size_class") == A.LARGE).any()
    info = g.find_partners_device("share", p_none, ap)
    assert info == {k: 0 for k in info}
    assert tuple(len(a) for a in g.download_partner_decisions(0)) == (0, 0, 0)
    refused(1, g.download_partner_decisions, 1)
    g.share_particles_device(p_none, ap)
    refused(1, g.share_particles_device, p_none, ap)                     # consumed
    twin = ffi.Context(product_lib, 70000, planes)
    twin.upload(mass, pos, vel)
    twin.step(p)
    twin.classify(p_none)
    twin.share_particles(p_none, ap, np.full(twin.n, A.MERGE_PARTNER_AVAILABLE, np.uint32), np.zeros(twin.n, np.uint16))
    same_fields(all_fields(g), all_fields(twin))
    twin.close()
    fresh_step()
    refused(1, g.merge_particles_device, p, ap)                          # lists, but no solution
    refused(1, g.find_partners_device, 2, p, ap)                         # kind
    refused(1, g.find_partners_device, "merge", None, ap)                # null params
    K = g.find_partners_device("share", p, ap)["participants"]
    assert K > 1
    before = all_fields(g)
    refused(1, g.merge_particles_device, p, ap)                          # the open solution is a share solution
    refused(1, g.download_partner_decisions, K + 1)                      # k != K
    refused(1, g.download_partner_decisions, K - 1)
    same_fields(before, all_fields(g))                                   # ... and nothing was modified
    assert len(g.download_partner_decisions(K)[0]) == K                  # the refusals left the solution open
    g.share_particles_device(p, ap)
    refused(1, g.share_particles_device, p, ap)                          # consumed: apply twice on one solution
    g.step(p)
    g.classify(p)
    # a solution made before sph_step / sph_upload / sph_merge_particles / a later problem, and applied after it
    g.find_partners_device("merge", p, ap)
    fresh_step()
    refused(1, g.merge_particles_device, p, ap)
    g.find_partners_device("merge", p, ap)
    g.upload(mass, pos, vel)
    refused(1, g.merge_particles_device, p, ap)
    fresh_step()
    g.find_partners_device("merge", p, ap)
    g.merge_particles(p, ap, np.full(g.n, A.MERGE_PARTNER_AVAILABLE, np.uint32), np.zeros(g.n, np.uint16))
    refused(1, g.merge_particles_device, p, ap)
    fresh_step()
    K = g.find_partners_device("merge", p, ap)["participants"]
    assert len(g.download_partner_problem("merge", p, ap, want_ids=True)[0]) == K
    refused(1, g.merge_particles_device, p, ap)                          # the later problem has no solution
    refused(1, g.download_partner_decisions, K)
    g.step(p)                                                            # a step after the refusals still works
    # the host may still decide on the problem a search opened
    g.classify(p)
    K = g.find_partners_device("merge", p, ap)["participants"]
    _, mp_c, mc_c = g.download_partner_decisions(K)
    g.merge_particles_compact(p, ap, mp_c, mc_c)
    assert g.n < len(mass)
    refused(1, g.merge_particles_device, p, ap)
    g.step(p)
    # a poisoned context (a NaN velocity trips a guard inside the step: a status of the library, no device fault): every call of the
    # header answers SPH_ERR_POISONED until sph_upload
    bad = vel.copy()
    bad[5, 0] = np.nan
    g.upload(mass, pos, bad)
    with pytest.raises(ffi.SphError) as e:
        g.step(p)
    assert e.value.status in (14, 15, 17, 18, 19)
    refused(31, g.find_partners_device, "share", p, ap)
    refused(31, g.download_partner_decisions, 0)
    refused(31, g.share_particles_device, p, ap)
    refused(31, g.merge_particles_device, p, ap)
    g.upload(mass, pos, vel)
    fresh_step()
    assert g.find_partners_device("merge", p, ap)["participants"] > 0
    g.merge_particles_device(p, ap)
    g.step(p)
    # a slab context (member of a loopback group): all four calls are unsupported, and the group steps afterwards
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 2)
    ffi.group_step(grp, p)
    refused(30, grp[0].find_partners_device, "share", p, ap)
    refused(30, grp[0].download_partner_decisions, 0)
    refused(30, grp[0].share_particles_device, p, ap)
    refused(30, grp[0].merge_particles_device, p, ap)
    ffi.group_step(grp, p)
