"""The partner searches of a slab group on the device (include/sph_slab_partner_search.h): the problem merged on the root against
distributed.merge_slab_partner_problems on the ranks' downloaded local problems, bit for bit; the decisions every member holds against
the sequential loop on that problem; the apply against sph_group_adapt_compact with the host's decisions on a twin group; whole adaptive
steps in export="device" against export="compact"; the refusals and the solution's lifetime.

Scenes are those of tests/test_gpu_slab_partner_problem.py -- the default scene (1 035 particles) on two ranks cut at the donor median,
where both kinds have foreign participants, and the two-size scene on three ranks, whose middle rank has ghosts on both sides -- plus
the default scene at half spacing (4 176 particles) on two ranks: n_global and the merge problem's K exceed the 2 048 words of a scan
tile, so the id-table scan and the row scan of the merge run over more than one tile.

The merge's error-word paths (two owners, differing bits, an entry that names nobody) are not reachable through a public call and are
not tested here."""
from pathlib import Path

import numpy as np
import pytest
import yaml

from adaptive_sph_amd import adaptivity as A, distributed as D, ffi, scene as sc
from adaptive_sph_amd.workloads import default_params
from tests.test_gpu_partner_search import NOBODY_LARGE, THRESHOLDS
from tests.test_gpu_slab_candidates import RADII, close_all, default_scene, full_lists, split_patterns
from tests.test_gpu_slab_partner_problem import (KINDS, PART_KEYS, assert_same_state, check_problem, refused, same_bits, state_by_id, three_rank_group,
                                                 three_rank_setup, two_rank_group)

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
SCAN_TILE = 2048
ALLOW = ("allow_share_with_optimal_particle", "allow_share_with_too_small_particle", "allow_merge_with_optimal_particle", "allow_merge_on_size_difference")


def find_against_the_host(lib, grp, P, p, dt, kind, label, merged, decisions, root=0, wide_threshold=0):
    """sph_group_find_partners_device on the state check_problem just examined: the merged problem on the root == `merged` (the numpy
    merge of the downloaded local problems), every member's decisions == `decisions` (the loop on that problem), the info == the numpy
    counts, the local counts == the prepare's.  -> info"""
    ap = A.adapt_params(P, dt)
    mp_c, mc_c = decisions
    info = ffi.group_find_partners_device(grp, kind, p, ap, wide_threshold=wide_threshold, root=root)
    parts = [c.slab_partner_problem_download() for c in grp]                 # the prepare inside the call left the same local problems
    assert info["ranks"] == [(len(q["ids"]), q["n_owned"], len(q["indices"])) for q in parts], (label, kind)
    again = D.merge_slab_partner_problems(parts)
    got = ffi.group_download_merged_partner_problem(grp)
    for key, a, b, c in zip(PART_KEYS, got, merged, again):
        assert same_bits(a, b) and same_bits(a, c), (label, kind, root, key)
    K = len(merged[0])
    for m in range(len(grp)):
        ids, mp, mc = ffi.group_download_partner_decisions(grp, m, K)
        assert np.array_equal(ids, merged[0]), (label, kind, root, m)
        assert np.array_equal(mp, mp_c) and np.array_equal(mc, mc_c), (label, kind, root, m, int(np.count_nonzero(mp != mp_c)))
    want = {"participants": K, "candidates": len(merged[7]), "donors": int(np.count_nonzero(mc_c)), "transfers": int(mc_c.sum())}
    assert {k: info[k] for k in want} == want, (label, kind, root, info)
    print(f"{label} {kind} root={root} threshold={wide_threshold:#x}: {info}")
    return info


@pytest.mark.parametrize("policy", ["fast", "exact"])
def test_merge_and_decisions_on_two_ranks(product_lib, policy):
    """The share behind the step, then -- behind the applied share, whose transfers left the ghosts stale until the prepare refreshes them
    -- the merge.  Each kind has foreign participants (reported by a rank that does not own them) and transfers."""
    P = default_params()
    p = P.to_ffi()
    grp, dt, num = two_rank_group(product_lib, P, policy)
    try:
        ap = A.adapt_params(P, dt)
        n = sum(c.n for c in grp)
        step_lists = full_lists(grp)
        merged, dec, foreign = check_problem(product_lib, grp, P, p, dt, "share", policy, step_lists)
        assert sum(foreign) > 0 and dec[1].sum() > 0
        before = state_by_id(grp, n)
        find_against_the_host(product_lib, grp, P, p, dt, "share", policy, merged, dec)
        assert_same_state(before, state_by_id(grp, n), "find + downloads")
        ffi.group_adapt_device(grp, "share", p, ap)
        assert not same_bits(before["mass"], D.gather_by_id(grp, "mass", n))
        merged, dec, foreign = check_problem(product_lib, grp, P, p, dt, "merge", f"{policy} behind the share", step_lists)
        assert sum(foreign) > 0 and dec[1].sum() > 0
        before = state_by_id(grp, n)
        find_against_the_host(product_lib, grp, P, p, dt, "merge", f"{policy} behind the share", merged, dec)
        assert_same_state(before, state_by_id(grp, n), "find + downloads behind the share")
        ffi.group_step(grp, p)                                       # an unused solution leaves the group able to step
    finally:
        close_all(grp)


def test_three_ranks_and_either_root(product_lib):
    """The middle rank reports participants of both neighbours; some participants are reported ONLY by ranks that do not own them (a
    candidate of a donor across the cut that is nobody's donor and no candidate at home): a merge that took the fields from the owner's
    report alone would leave them empty.  The same problem, decisions and info whether rank 0 or the middle rank merges."""
    P, scene = three_rank_setup()
    p = P.to_ffi()
    grp, dt, num = three_rank_group(product_lib, P, scene)
    try:
        only_foreign = {kind: 0 for kind in KINDS}
        for kind in KINDS:
            for allow in (False, True):
                Pa = P.replace(**{a: allow for a in ALLOW})
                merged, dec, foreign = check_problem(product_lib, grp, Pa, p, dt, kind, f"three ranks allow={allow}")
                parts = [c.slab_partner_problem_download() for c in grp]
                owned = np.concatenate([q["ids"][:q["n_owned"]] for q in parts])
                only_foreign[kind] += len(np.setdiff1d(merged[0], owned))
                infos = [find_against_the_host(product_lib, grp, Pa, p, dt, kind, f"three ranks allow={allow}", merged, dec, root=root) for root in (0, 1)]
                assert infos[0] == infos[1], (kind, allow)
        print(f"participants reported only as foreign: {only_foreign}")
        assert sum(only_foreign.values()) > 0, only_foreign
        ffi.group_step(grp, p)
    finally:
        close_all(grp)


def test_more_than_one_scan_tile(product_lib):
    """The default scene at half spacing on two ranks: n_global = 4 176 and the merge problem's K > 2 048.  Every wide threshold: the same
    merged problem, the same decisions, the same schedule."""
    doc = yaml.safe_load((REPO / "tests" / "golden" / "default-scene.yaml").read_text())
    for b in doc["blocks"]:
        b["spacing"] = b["spacing"] * 0.5
    scn = sc.SceneConfig.from_mapping(doc)
    pos, mass, vel = sc.init_particles(scn)
    assert len(mass) == 4176
    P = default_params(**RADII)
    p = P.to_ffi()
    grp = D.make_loopback_group(product_lib, pos, mass, vel, sc.boundary_planes(scn.boundary, P.init_boundary_handler), 2)
    try:
        for _ in range(2):
            sts = ffi.group_step(grp, p)
        dt = float(sts[0].dt)
        for kind in ("merge", "share"):
            merged, dec, _ = check_problem(product_lib, grp, P, p, dt, kind, "half spacing")
            infos = [find_against_the_host(product_lib, grp, P, p, dt, kind, "half spacing", merged, dec, wide_threshold=thr) for thr in THRESHOLDS]
            assert infos[1]["wide_rounds"] == infos[1]["rounds"] and infos[2]["wide_rounds"] == 0
            assert len({(i["rounds"], i["max_frontier"]) for i in infos}) == 1, infos
            if kind == "merge":
                assert len(merged[0]) > SCAN_TILE and sum(c.n for c in grp) > SCAN_TILE and infos[0]["transfers"] > 0, len(merged[0])
        ffi.group_step(grp, p)
    finally:
        close_all(grp)


@pytest.mark.parametrize("case", ["share", "merge", "nobody"])
def test_the_device_apply_equals_the_compact_apply(product_lib, case):
    """Twin groups: one applies the open solution (sph_group_adapt_device), the other the host's decisions on the merged problem
    (sph_group_adapt_compact).  Every downloadable field, the ids and the per-rank counts, bit for bit, and again after one more step.
    "merge": behind the share, with deletions (the vector is renumbered); "nobody": params under which no particle is Large -- K == 0,
    an open solution without decisions, the apply of all-AVAILABLE arrays."""
    P = default_params()
    p = P.to_ffi()
    a, dt, num = two_rank_group(product_lib, P)
    b, dt_b, _ = two_rank_group(product_lib, P)
    try:
        assert dt == dt_b
        ap = A.adapt_params(P, dt)
        n = sum(c.n for c in a)
        step_lists = full_lists(b)
        if case == "nobody":
            Pn = default_params(**NOBODY_LARGE)
            pn, apn = Pn.to_ffi(), A.adapt_params(Pn, dt)
            for c in a + b:
                c.classify(pn)
            info = ffi.group_find_partners_device(a, "share", pn, apn)
            assert info == {"participants": 0, "candidates": 0, "donors": 0, "transfers": 0, "rounds": 0, "max_frontier": 0, "wide_rounds": 0, "ranks": [(0, 0, 0)] * 2}
            assert all(len(v) == 0 for v in ffi.group_download_partner_decisions(a, 1, 0))
            assert len(ffi.group_download_merged_partner_problem(a)[0]) == 0
            ffi.group_adapt_device(a, "share", pn, apn)
            none = (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint16))
            ffi.group_adapt_compact(b, "share", pn, apn, *none)
        else:
            kinds = ("share",) if case == "share" else ("share", "merge")
            for kind in kinds:
                for c in a:
                    c.classify(p)
                info = ffi.group_find_partners_device(a, kind, p, ap)
                (pids, *_), (mp_c, mc_c), _ = check_problem(product_lib, b, P, p, dt, kind, case, step_lists)
                assert info["participants"] == len(pids) and info["transfers"] == int(mc_c.sum()) > 0
                ffi.group_adapt_device(a, kind, p, ap)
                ffi.group_adapt_compact(b, kind, p, ap, pids, mp_c, mc_c)
        n_after = sum(c.n for c in a)
        assert [c.n for c in a] == [c.n for c in b]
        assert n_after < n if case == "merge" else n_after == n
        assert_same_state(state_by_id(a, n_after), state_by_id(b, n_after), case)
        for grp in (a, b):
            ffi.group_step(grp, p)
        assert_same_state(state_by_id(a, n_after), state_by_id(b, n_after), case + " + step")
    finally:
        close_all(a + b)


def test_whole_adaptive_steps_equal_the_compact_mode(product_lib):
    """Twin groups in lockstep over eight adaptive steps of the default configuration, one in export="compact", one in export="device":
    the same events and bit-identical states after every step, while the splits grow the vector past 4 000 particles.  What the device
    mode reports as moved: 48 B per search and the 8 B mass sums down, nothing up."""
    P = default_params()
    pos, mass, vel, planes = default_scene(P)
    p = P.to_ffi()
    k = 2
    twins = {}
    seen = {"shares": 0, "merges": 0, "splits": 0}
    n_max = 0
    try:
        for mode in ("compact", "device"):
            twins[mode] = D.make_loopback_group(product_lib, pos, mass, vel, planes, k)
            for c in twins[mode]:
                c.set_split_patterns(split_patterns().patterns)
        for s in range(1, 9):
            info = {}
            for mode, grp in twins.items():
                sts = ffi.group_step(grp, p)
                info[mode] = D.group_single_step_adaptivity_on_slabs(product_lib, grp, P, float(sts[0].dt), int(sts[0].step_number), export=mode)
                assert info[mode]["export"] == mode
            ic, io = info["compact"], info["device"]
            for key in ("n_before", "n_after", "shares", "merges", "splits", "participants", "exported_indices"):
                assert ic[key] == io[key], (s, key, ic[key], io[key])
            for key in seen:
                seen[key] += io[key]
            assert [(q["kind"], q["participants"], q["ranks"]) for q in ic["passes"]] == [(q["kind"], q["participants"], [tuple(r) for r in q["ranks"]]) for q in io["passes"]]
            assert all({"rounds", "max_frontier", "wide_rounds"} <= set(q) for q in io["passes"])
            assert io["bytes_down"] == 48 * len(io["passes"]) + 2 * 8 * k and io["bytes_up"] == 0
            between = sum(25 * K + 4 * (Ko + 1) + 4 * T for q in io["passes"] for r, (K, Ko, T) in enumerate(q["ranks"]) if r != 0 and K) \
                + sum(10 * q["participants"] * (k - 1) for q in io["passes"])
            assert io["bytes_between_devices"] == between
            n = io["n_after"]
            n_max = max(n_max, n)
            print(f"step {s}: n={n} {[(q['kind'], q['participants'], q['rounds'], q['max_frontier'], q['wide_rounds']) for q in io['passes']]} bytes down compact "
                  f"{ic['bytes_down']} up {ic['bytes_up']} / device down {io['bytes_down']} between devices {io['bytes_between_devices']}")
            assert_same_state(state_by_id(twins["compact"], n), state_by_id(twins["device"], n), f"step {s}")
        assert all(v > 0 for v in seen.values()), seen
        assert n_max > 4000, n_max
    finally:
        for grp in twins.values():
            close_all(grp)


def test_refusals_and_lifetime(product_lib):
    P = default_params(**RADII)
    pos, mass, vel, planes = default_scene(P)
    p = P.to_ffi()
    ap = A.adapt_params(P, 1e-3)
    plain = ffi.Context(product_lib, 70000, planes)
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 2)
    find, adapt, decisions, problem = ffi.group_find_partners_device, ffi.group_adapt_device, ffi.group_download_partner_decisions, ffi.group_download_merged_partner_problem
    try:
        for c in grp:
            c.set_split_patterns(split_patterns().patterns)
        plain.upload(mass, pos, vel)
        plain.step(p)
        plain.classify(p)
        # a plain context: alone, and among slab contexts
        for ctxs in ([plain], [grp[0], plain]):
            refused(30, find, ctxs, "share", p, ap)
            refused(30, adapt, ctxs, "share", p, ap)
            refused(30, decisions, ctxs, 0, 0)
            refused(30, problem, ctxs)
        plain.step(p)
        refused(1, find, grp, "share", p, ap)                        # no step before (the prepare's refusal)
        sts = ffi.group_step(grp, p)
        dt = float(sts[0].dt)
        ap = A.adapt_params(P, dt)
        n = len(mass)
        for c in grp:
            c.classify(p)
        state0 = state_by_id(grp, n)
        refused(1, adapt, grp, "share", p, ap)                       # nothing found yet
        refused(1, decisions, grp, 0, 0)
        refused(1, problem, grp)
        refused(1, find, grp, "share", p, ap, 0, 2)                  # root outside 0 .. n-1
        refused(1, find, grp, "share", p, ap, 0, -1)
        refused(1, find, grp, 2, p, ap)                              # kind
        refused(1, find, grp, "share", None, ap)
        refused(1, find, grp, "share", p, None)
        import ctypes as C
        h2 = (C.c_void_p * 2)(grp[0].handle, grp[1].handle)
        assert product_lib.group_find_partners_device(h2, 2, 0, C.byref(p), C.byref(ap), 0, 0, None, None, None, None) == 1   # info NULL
        refused(1, find, grp[::-1], "share", p, ap)                  # not ranks 0 .. n-1 in order
        refused(1, find, grp[:1], "share", p, ap)                    # one context of a group of two
        refused(1, adapt, grp, "share", p, ap)                       # the refused calls opened nothing
        assert_same_state(state0, state_by_id(grp, n), "refused finds")
        # an open solution: its kind, its K, its members
        info = find(grp, "share", p, ap, 0, 1)
        K = info["participants"]
        assert K > 0 and info["transfers"] > 0
        refused(1, adapt, grp, "merge", p, ap)                       # a solution of the other kind
        refused(1, adapt, grp, 2, p, ap)                             # op
        refused(1, adapt, grp, "share", None, ap)
        refused(1, adapt, grp, "share", p, None)
        refused(1, decisions, grp, 0, K + 1)                         # k != K
        refused(1, decisions, grp, 2, K)                             # from_member outside 0 .. n-1
        refused(1, adapt, grp[::-1], "share", p, ap)
        assert_same_state(state0, state_by_id(grp, n), "refused applies")
        sol = decisions(grp, 0, K)
        assert all(np.array_equal(x, y) for x, y in zip(sol, decisions(grp, 1, K)))
        adapt(grp, "share", p, ap)                                   # the refusals left it open
        assert not same_bits(state0["mass"], D.gather_by_id(grp, "mass", n))
        refused(1, adapt, grp, "share", p, ap)                       # consumed by its own apply (the share left the prepared rows open)
        refused(1, decisions, grp, 0, K)
        refused(1, problem, grp)
        grp[0].slab_partner_problem_download()
        # closed by a later prepare
        for c in grp:
            c.classify(p)
        info = find(grp, "merge", p, ap)
        ffi.group_slab_partner_problem_prepare(grp, "merge", p, ap)
        refused(1, adapt, grp, "merge", p, ap)
        info = find(grp, "merge", p, ap)
        ffi.group_slab_candidates_prepare(grp, "merge", p, ap)
        refused(1, adapt, grp, "merge", p, ap)
        # closed by a step
        info = find(grp, "merge", p, ap)
        sts = ffi.group_step(grp, p)
        ap = A.adapt_params(P, float(sts[0].dt))
        refused(1, adapt, grp, "merge", p, ap)
        refused(1, decisions, grp, 0, info["participants"])
        # closed by an upload_field of mass on one member: the group's solution is every member's
        for c in grp:
            c.classify(p)
        info = find(grp, "share", p, ap)
        grp[1].upload_field("mass", grp[1].download("mass"))
        refused(1, adapt, grp, "share", p, ap)
        refused(1, problem, grp)
        sts = ffi.group_step(grp, p)
        ap = A.adapt_params(P, float(sts[0].dt))
        # closed by an upload
        for c in grp:
            c.classify(p)
        info = find(grp, "share", p, ap)
        ids0 = grp[0].download("particle_id")
        m0, x0, v0 = grp[0].download("mass"), grp[0].download("position"), grp[0].download("velocity")
        grp[0].upload(m0, x0, v0)
        grp[0].upload_field("particle_id", ids0)
        refused(1, adapt, grp, "share", p, ap)
        refused(1, decisions, grp, 1, info["participants"])
        ffi.group_step(grp, p)                                       # every refusal left the group able to step
    finally:
        plain.close()
        close_all(grp)


def test_a_poisoned_member(product_lib):
    """A group poisoned by a step that ran out of room (tests/test_gpu_slab_partner_problem.py) answers SPH_ERR_POISONED."""
    from adaptive_sph_amd.workloads import dam_break_params
    scn = sc.dam_break_small(96, 48, 1 / 48)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    P = dam_break_params(max_iters=3, level_estimation_method="EmptyAngle", maximum_surface_distance=0.2, particle_radius_fine=0.004, particle_radius_base=0.02)
    p = P.to_ffi()
    ap = A.adapt_params(P, 1e-3)
    cuts = D.slab_cuts(pos[:, 0], 2)
    parts = D.partition(pos[:, 0], cuts)
    grp = []
    try:
        for r in range(2):
            c = ffi.Context(product_lib, len(parts[r]) + 8, planes)
            c.dist_configure(r, 2, cuts[r], cuts[r + 1])
            c.upload(mass[parts[r]], pos[parts[r]], vel[parts[r]])
            c.upload_field("particle_id", parts[r].astype(np.uint32))
            grp.append(c)
        with pytest.raises(ffi.SphError) as e:
            for _ in range(3):
                ffi.group_step(grp, p)
        assert e.value.status == 3
        refused(31, ffi.group_find_partners_device, grp, "share", p, ap)
        refused(31, ffi.group_adapt_device, grp, "share", p, ap)
        refused(31, ffi.group_download_partner_decisions, grp, 0, 0)
        refused(31, ffi.group_download_merged_partner_problem, grp)
    finally:
        close_all(grp)
