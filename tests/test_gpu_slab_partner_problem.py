"""The compact partner problem on slab contexts (include/sph_slab_partner_problem.h): every rank's local problem against the numpy
contract adaptivity.slab_partner_problem_reference, the merged problem against adaptivity.partner_problem_reference on the gathered
fields and the assembled full lists, the apply from K decisions against sph_group_adapt on the expanded arrays, whole adaptive steps in
export="compact" against export="candidates" (loopback group and one thread per rank), the snapshot, and the refusals.

Scenes: the default scene (1 035 particles) in its second step on two ranks cut at the median x of the donors with candidates -- there
the numpy contract alone has foreign participants in both kinds (FAST: 2 + 2 in the share problem of 204, 32 + 34 in the merge problem
of 200 behind the share) --; the two-size scene of the sort tests on three ranks, whose middle rank has a ghost layer on either side -- the smallest shapes where rows
cross a cut on both sides of a rank."""
import numpy as np
import pytest

from adaptive_sph_amd import adaptivity as A, distributed as D, ffi, scene as sc
from adaptive_sph_amd.workloads import dam_break_params, default_params
from tests.test_gpu_adaptivity import _fields_by_id
from tests.test_gpu_incremental_sort import two_sizes_scene
from tests.test_gpu_slab_candidates import (RADII, _Threads, adapt_on_threads, close_all, cut_group, default_scene, donor_median_x, full_lists, gathered,
                                            split_patterns)

pytestmark = pytest.mark.gpu
FIELDS = ffi.PROBLEM_FIELDS
KINDS = ("share", "merge")
PART_KEYS = ("ids",) + tuple(FIELDS) + ("offsets", "indices")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def state_by_id(grp, n):
    """every downloadable field adaptivity writes, by global id, and which rank holds which ids"""
    f = _fields_by_id(grp, n)
    f["h2"] = D.gather_by_id(grp, "h2", n)
    f["owner"] = D.gather_by_id(grp, "particle_id", n)
    for r, c in enumerate(grp):
        f["owner"][c.download("particle_id")] = r
    return f


def assert_same_state(a, b, label):
    assert a.keys() == b.keys()
    for f in a:
        assert same_bits(a[f], b[f]), (label, f)


def two_rank_group(lib, P, policy=None):
    """the default scene on two loopback ranks cut at the donor median (of the first step), two steps -> (group, dt, step number)"""
    scene = default_scene(P)
    p = P.to_ffi()
    cut, xs = donor_median_x(lib, P, scene, 1, policy)
    grp, sts, _ = cut_group(lib, scene, P, p, 2, cut, xs, policy)
    try:
        sts = ffi.group_step(grp, p)
    except Exception:
        close_all(grp)
        raise
    return grp, float(sts[0].dt), int(sts[0].step_number)


def three_rank_setup():
    scn = two_sizes_scene()
    pos, mass, vel = sc.init_particles(scn)
    r_fine = float(np.sqrt(np.float32(0.02) ** 2 * 0.93 / np.pi))
    P = dam_break_params(level_estimation_method="EmptyAngle", particle_radius_fine=r_fine, particle_radius_base=4 * r_fine, maximum_surface_distance=0.3,
                         max_iters=6)
    return P, (pos, mass, vel, sc.boundary_planes(scn.boundary, P.init_boundary_handler))


def three_rank_group(lib, P, scene):
    """tests/test_gpu_slab_candidates.py::test_three_ranks_with_ghosts_on_both_sides: the first pair of cuts the group accepts, three steps"""
    pos, mass, vel, planes = scene
    p = P.to_ffi()
    last = None
    for c1, c2 in [(a, b) for b in (-0.39, -0.40, -0.38) for a in (-0.83, -0.85, -0.82, -0.87)]:
        grp = D.make_loopback_group(lib, pos, mass, vel, planes, 3, cuts=[-D.INF, c1, c2, D.INF])
        try:
            for _ in range(3):
                sts = ffi.group_step(grp, p)
            return grp, float(sts[0].dt), int(sts[0].step_number)
        except ffi.SphError as e:
            close_all(grp)
            last = e
            if e.status != 30:
                raise
    raise last


def check_problem(lib, grp, P, p, dt, kind, label, step_lists=None):
    """prepare `kind` on the group's current state; every rank's local problem against the numpy contract, the merged problem against
    partner_problem_reference.  `step_lists`: full_lists(grp) from before a share (the lists cannot be exported behind one).
    -> (merged problem, its decisions in compact ids, foreign participants per rank)"""
    ap = A.adapt_params(P, dt)
    ids, n, lists = step_lists or full_lists(grp)
    f = gathered(grp, n, p)
    counts = ffi.group_slab_partner_problem_prepare(grp, kind, p, ap)
    parts = [c.slab_partner_problem_download() for c in grp]
    foreign = []
    for r, (c, q, (K, Ko, T)) in enumerate(zip(grp, parts, counts)):
        off, idx = c.slab_candidates_download(counts=(c.n, T))          # the rows the prepare left: the problem is packed from them
        ref = A.slab_partner_problem_reference(ids[r], off, idx, *[f[k] for k in FIELDS])
        assert (K, Ko, T) == (len(q["ids"]), q["n_owned"], len(q["indices"])) == (len(ref["ids"]), ref["n_owned"], len(ref["indices"])), (label, kind, r)
        assert same_bits(q["offsets"], ref["offsets"]) and same_bits(q["indices"], ref["indices"]) and same_bits(q["indices"], idx), (label, kind, r)
        order = np.concatenate([np.arange(Ko), Ko + np.argsort(q["ids"][Ko:], kind="stable")]).astype(np.int64)   # foreign ones by id
        for key in ("ids",) + tuple(FIELDS):
            assert same_bits(q[key][order], ref[key]), (label, kind, r, key)
        foreign.append(K - Ko)
    merged = D.merge_slab_partner_problems(parts)
    want = A.partner_problem_reference(kind, *[f[k] for k in FIELDS], lists[0], lists[1], P)
    for key, a, b in zip(PART_KEYS, merged, want):
        assert same_bits(a, b), (label, kind, key)
    K = len(merged[0])
    print(f"{label} {kind}: n={n} K={K} candidates={len(merged[7])} local (K, owned, candidates)={counts} foreign={foreign}")
    assert K < n, (label, kind, K, n)
    pids, *fields, off_c, idx_c = merged
    mp_c, mc_c = D._decide_compact(lib, kind, pids, fields, off_c, idx_c, P, dt)
    full = D._decide_on_gathered(lib, kind, f, lists, P, dt)
    mp, mc = A.expand_partner_decisions(n, pids, mp_c, mc_c)
    assert np.array_equal(full[0], mp) and np.array_equal(full[1], mc), (label, kind)
    return merged, (mp_c.copy(), mc_c.copy()), foreign


@pytest.mark.parametrize("policy,after", [("fast", False), ("exact", False), ("fast", True)])
def test_local_and_merged_problem_equal_the_numpy_contract(product_lib, policy, after):
    """Two ranks: the share problem behind the step, then -- behind the applied share, whose transfers left the ghosts stale -- the merge
    problem: a ghost's packed mass and level are its owner's values after the share, bit for bit (the reference takes them from the
    owners' downloads).  Each kind must have a foreign participant: without one no ghost record was packed."""
    P = default_params(level_estimation_after_advection=after)
    p = P.to_ffi()
    grp, dt, num = two_rank_group(product_lib, P, policy)
    try:
        label = f"[{policy}, after={after}]"
        step_lists = full_lists(grp)
        (pids, *_), (mp_c, mc_c), foreign = check_problem(product_lib, grp, P, p, dt, "share", label, step_lists)
        assert len(pids) > 0 and sum(foreign) > 0, (len(pids), foreign)
        assert mc_c.sum() > 0
        ffi.group_adapt_compact(grp, "share", p, A.adapt_params(P, dt), pids, mp_c, mc_c)
        (mids, *_), _, foreign = check_problem(product_lib, grp, P, p, dt, "merge", label + f" behind {int(mc_c.sum())} shares", step_lists)
        assert len(mids) > 0 and sum(foreign) > 0, (len(mids), foreign)
        ffi.group_step(grp, p)                                       # the export left the group able to step
    finally:
        close_all(grp)


def test_three_ranks_with_ghosts_on_both_sides(product_lib):
    """The middle rank packs foreign participants from both neighbours.  Both settings of the allow_* flags, as the candidate rows'
    test on this scene: each kind has participants, and foreign ones, under at least one of them."""
    P, scene = three_rank_setup()
    p = P.to_ffi()
    grp, dt, num = three_rank_group(product_lib, P, scene)
    try:
        ids, n, _ = full_lists(grp)
        owner = np.empty(n, np.int64)
        for r, i in enumerate(ids):
            owner[i] = r
        sides = set()
        size = {kind: 0 for kind in KINDS}
        across = {kind: 0 for kind in KINDS}
        for kind in KINDS:
            for allow in (False, True):
                Pa = P.replace(**{a: allow for a in ("allow_share_with_optimal_particle", "allow_share_with_too_small_particle",
                                                     "allow_merge_with_optimal_particle", "allow_merge_on_size_difference")})
                (pids, *_), _, foreign = check_problem(product_lib, grp, Pa, p, dt, kind, f"three ranks allow={allow}")
                size[kind] += len(pids)
                across[kind] += sum(foreign)
                q = grp[1].slab_partner_problem_download()
                sides |= {int(o) for o in owner[q["ids"][q["n_owned"]:]]}
        assert all(v > 0 for v in size.values()) and all(v > 0 for v in across.values()), (size, across)
        assert sides == {0, 2}, sides
        ffi.group_step(grp, p)
    finally:
        close_all(grp)


@pytest.mark.parametrize("case", ["share", "merge", "merge_nothing"])
def test_the_compact_apply_equals_the_apply_of_the_expanded_arrays(product_lib, case):
    """Twin groups: one takes the K decisions (sph_group_adapt_compact), the other merge_partner / merge_counter of the whole vector
    expanded from them (sph_group_adapt).  Every downloadable field and the ids on every rank, bit for bit.  "merge": behind the share,
    with deletions (the vector is renumbered); "merge_nothing": K participants, nobody decided."""
    P = default_params()
    p = P.to_ffi()
    a, dt, num = two_rank_group(product_lib, P)
    b, dt_b, _ = two_rank_group(product_lib, P)
    try:
        assert dt == dt_b
        ap = A.adapt_params(P, dt)
        n = sum(c.n for c in a)
        kind = "share" if case == "share" else "merge"
        step_lists = full_lists(a)
        if case == "merge":                                          # both behind the same share
            (pids, *_), (mp_c, mc_c), _ = check_problem(product_lib, a, P, p, dt, "share", case, step_lists)
            for grp in (a, b):
                ffi.group_adapt(grp, "share", p, ap, *A.expand_partner_decisions(n, pids, mp_c, mc_c))
        (pids, *_), (mp_c, mc_c), _ = check_problem(product_lib, a, P, p, dt, kind, case, step_lists)
        for c in b:
            c.classify(p)                                            # (check_problem classified the other twin)
        if case == "merge_nothing":
            mp_c[:], mc_c[:] = A.MERGE_PARTNER_AVAILABLE, 0
        else:
            assert mc_c.sum() > 0
        ffi.group_adapt_compact(a, kind, p, ap, pids, mp_c, mc_c)
        ffi.group_adapt(b, kind, p, ap, *A.expand_partner_decisions(n, pids, mp_c, mc_c))
        n_after = sum(c.n for c in a)
        assert n_after == sum(c.n for c in b) and [c.n for c in a] == [c.n for c in b]
        if case == "merge":
            assert n_after < n                                       # deletions
        else:
            assert n_after == n
        assert_same_state(state_by_id(a, n_after), state_by_id(b, n_after), case)
        for grp in (a, b):
            ffi.group_step(grp, p)
        assert_same_state(state_by_id(a, n_after), state_by_id(b, n_after), case + " + step")
    finally:
        close_all(a + b)


def compact_on_threads(lib, th, P, dt, num, passes):
    """single_step_adaptivity in compact mode with the per-rank entry points, every collective from k threads"""
    b = th.grp
    p, ap = P.to_ffi(), A.adapt_params(P, dt)
    n = int(sum(c.n for c in b))
    info = {"shares": 0, "merges": 0, "splits": 0}

    def search(kind):
        th.all(lambda c: c.classify(p))
        th.all(lambda c: c.slab_partner_problem_prepare(kind, p, ap))
        pids, *fields, off_c, idx_c = D.merge_slab_partner_problems([c.slab_partner_problem_download() for c in b])
        mp_c, mc_c = D._decide_compact(lib, kind, pids, fields, off_c, idx_c, P, dt)
        passes.append((kind,) + A.expand_partner_decisions(n, pids, mp_c, mc_c))
        return pids, mp_c, mc_c

    if P.sharing:
        pids, mp_c, mc_c = search("share")
        info["shares"] = int(mc_c.sum())
        th.all(lambda c: c.slab_share_particles_compact(p, ap, pids, mp_c, mc_c))
    if num % 2 == 0:
        pids, mp_c, mc_c = search("merge")
        info["merges"] = int(mc_c.sum())
        th.all(lambda c: c.slab_merge_particles_compact(p, ap, pids, mp_c, mc_c))
    else:
        th.all(lambda c: c.classify(p))
        th.all(lambda c: c.split_particles(p, ap))
        info["splits"] = int(sum(c.n for c in b)) - n
    return info


@pytest.mark.parametrize("transport", ["loopback", "threads"])
def test_whole_adaptive_steps_equal_the_candidates_mode(product_lib, monkeypatch, transport):
    """Twin groups in lockstep over three steps -- share + split, share + merge, share + split --, one in export="candidates", one in
    export="compact": the same merge_partner / merge_counter in every pass, bit-identical states after every adaptive step.  Loopback:
    the drivers themselves, and what they report as moved.  Threads: the per-rank entry points, each rank on a thread of its own."""
    P = default_params(**RADII)
    pos, mass, vel, planes = default_scene(P)
    p = P.to_ffi()
    k = 2
    passes = {"candidates": [], "compact": []}
    current = [None]
    inner_full, inner_compact = D._decide_on_gathered, D._decide_compact

    def rec_full(lib, kind, g, lists, P_, dt_):
        mp, mc = inner_full(lib, kind, g, lists, P_, dt_)
        passes[current[0]].append((kind, mp.copy(), mc.copy()))
        return mp, mc

    def rec_compact(lib, kind, ids, fields, off_c, idx_c, P_, dt_):
        mp_c, mc_c = inner_compact(lib, kind, ids, fields, off_c, idx_c, P_, dt_)
        passes[current[0]].append((kind,) + A.expand_partner_decisions(current[1], ids, mp_c, mc_c))
        return mp_c, mc_c

    twins, closers = {}, []
    seen = {"shares": 0, "merges": 0, "splits": 0}
    try:
        for mode in passes:
            if transport == "threads":
                tg = D.ThreadedGroup(product_lib, pos, mass, vel, planes, k)
                closers.append(tg.close)
                twins[mode] = (tg.contexts, tg.step, _Threads(tg.contexts))
                closers.append(twins[mode][2].close)
            else:
                grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, k)
                closers.append(lambda grp=grp: close_all(grp))
                twins[mode] = (grp, lambda p_, grp=grp: ffi.group_step(grp, p_), None)
            for c in twins[mode][0]:
                c.set_split_patterns(split_patterns().patterns)
        if transport == "loopback":
            monkeypatch.setattr(D, "_decide_on_gathered", rec_full)
            monkeypatch.setattr(D, "_decide_compact", rec_compact)
        for s in range(1, 4):
            info = {}
            for mode, (grp, step, th) in twins.items():
                sts = step(p)
                dt, num = float(sts[0].dt), int(sts[0].step_number)
                current[:] = [mode, sum(c.n for c in grp)]
                if th is None:
                    info[mode] = D.group_single_step_adaptivity_on_slabs(product_lib, grp, P, dt, num, export=mode)
                    assert info[mode]["export"] == mode
                elif mode == "compact":
                    info[mode] = compact_on_threads(product_lib, th, P, dt, num, passes[mode])
                else:
                    info[mode] = adapt_on_threads(product_lib, th, P, dt, num, mode, passes[mode])
            ca, co = passes["candidates"], passes["compact"]
            assert len(ca) == len(co) == (2 if num % 2 == 0 else 1), (s, num, len(ca), len(co))
            for (k1, mp1, mc1), (k2, mp2, mc2) in zip(ca, co):
                assert k1 == k2 and np.array_equal(mp1, mp2) and np.array_equal(mc1, mc2), (s, k1)
            ca.clear()
            co.clear()
            for key in seen:
                assert info["candidates"][key] == info["compact"][key], (s, key)
                seen[key] += info["compact"][key]
            if transport == "loopback":
                ic, io = info["candidates"], info["compact"]
                down = sum(25 * K + 4 * (Ko + 1) + 4 * T for q in io["passes"] for K, Ko, T in q["ranks"]) + 2 * 8 * k
                print(f"step {s}: participants {io['participants']} in {len(io['passes'])} passes, bytes down candidates {ic['bytes_down']} / compact "
                      f"{io['bytes_down']}, bytes up compact {io['bytes_up']} (whole arrays: {6 * ic['n_before'] * k} per pass)")
                assert io["bytes_down"] == down and io["bytes_up"] == 10 * k * io["participants"]
                assert io["participants"] == sum(q["participants"] for q in io["passes"]) > 0
                assert io["exported_indices"] == ic["exported_indices"]
                assert io["bytes_down"] < ic["bytes_down"]
            n = sum(c.n for c in twins["compact"][0])
            assert n == sum(c.n for c in twins["candidates"][0])
            assert_same_state(state_by_id(twins["candidates"][0], n), state_by_id(twins["compact"][0], n), f"step {s}")
        assert all(v > 0 for v in seen.values()), seen
        for grp, step, th in twins.values():
            step(p)
    finally:
        for f in reversed(closers):
            f()


def test_the_download_is_a_snapshot_and_the_prepare_writes_nothing(product_lib):
    """Two downloads of one prepared problem: the same bytes.  The prepare (both kinds) changes no field of any owned particle.  Behind
    the share that follows, the download still returns what was packed -- while the masses on the device have changed."""
    P = default_params()
    p = P.to_ffi()
    a, dt, num = two_rank_group(product_lib, P)
    try:
        ap = A.adapt_params(P, dt)
        n = sum(c.n for c in a)
        for c in a:
            c.classify(p)
        before = state_by_id(a, n)
        ffi.group_slab_partner_problem_prepare(a, "merge", p, ap)
        ffi.group_slab_partner_problem_prepare(a, "share", p, ap)
        assert_same_state(before, state_by_id(a, n), "prepare")
        first = [c.slab_partner_problem_download() for c in a]
        second = [c.slab_partner_problem_download() for c in a]
        assert sum(len(q["ids"]) for q in first) > 0
        for q1, q2 in zip(first, second):
            assert q1["n_owned"] == q2["n_owned"] and all(same_bits(q1[key], q2[key]) for key in PART_KEYS)
        pids, *fields, off_c, idx_c = D.merge_slab_partner_problems(first)
        mp_c, mc_c = D._decide_compact(product_lib, "share", pids, fields, off_c, idx_c, P, dt)
        assert mc_c.sum() > 0
        ffi.group_adapt_compact(a, "share", p, ap, pids, mp_c, mc_c)
        assert not same_bits(before["mass"], D.gather_by_id(a, "mass", n))
        for q1, c in zip(first, a):
            q3 = c.slab_partner_problem_download()
            assert q1["n_owned"] == q3["n_owned"] and all(same_bits(q1[key], q3[key]) for key in PART_KEYS)
        ffi.group_step(a, p)
    finally:
        close_all(a)


def refused(status, f, *args):
    with pytest.raises(ffi.SphError) as e:
        f(*args)
    assert e.value.status == status, e.value


def test_refusals(product_lib):
    P = default_params(**RADII)
    pos, mass, vel, planes = default_scene(P)
    p = P.to_ffi()
    ap = A.adapt_params(P, 1e-3)
    none = (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint16))
    plain = ffi.Context(product_lib, 70000, planes)
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 2)
    try:
        for c in grp:
            c.set_split_patterns(split_patterns().patterns)
        plain.upload(mass, pos, vel)
        plain.step(p)
        plain.classify(p)
        before = {f: plain.download(f) for f in ("mass", "position", "velocity", "h2", "level_estimation", "particle_size_class")}
        refused(30, plain.slab_partner_problem_prepare, "share", p, ap)      # a plain context
        refused(30, plain.slab_partner_problem_download)
        refused(30, plain.slab_share_particles_compact, p, ap, *none)
        refused(30, plain.slab_merge_particles_compact, p, ap, *none)
        for f, v in before.items():
            assert same_bits(v, plain.download(f)), f
        plain.step(p)
        refused(1, ffi.group_slab_partner_problem_prepare, grp, "share", p, ap)   # no step before
        refused(1, grp[0].slab_partner_problem_download)                         # nothing prepared
        sts = ffi.group_step(grp, p)
        dt = float(sts[0].dt)
        ap = A.adapt_params(P, dt)
        n = len(mass)
        for c in grp:
            c.classify(p)
        refused(1, ffi.group_slab_partner_problem_prepare, grp, 2, p, ap)        # kind
        refused(1, ffi.group_slab_partner_problem_prepare, grp, "merge", None, ap)
        refused(1, ffi.group_slab_partner_problem_prepare, grp, "merge", p, None)
        refused(1, grp[0].slab_partner_problem_download)                         # the refusals prepared nothing
        refused(30, grp[0].share_particles_compact, p, ap, none[1], none[2])     # sph_share_particles_compact still refuses a slab context
        refused(30, grp[0].merge_particles_compact, p, ap, none[1], none[2])
        refused(30, grp[0].download_partner_problem, "share", p, ap)
        state0 = state_by_id(grp, n)
        counts = ffi.group_slab_partner_problem_prepare(grp, "merge", p, ap)
        r = max(range(2), key=lambda i: counts[i][2])
        K, Ko, T = counts[r]
        assert K > 1 and T > 1 and 0 < Ko <= K
        # capacities one short: refused with the counts set, the problem stays prepared
        import ctypes as C
        k_, ko_, t_ = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        short_ids, short_idx = np.empty(K - 1, np.uint32), np.empty(T - 1, np.uint32)
        dl = product_lib.slab_partner_problem_download
        h = grp[r].handle
        assert dl(h, short_ids.ctypes.data, None, None, None, None, None, None, K - 1, None, 0, C.byref(k_), C.byref(ko_), C.byref(t_)) == 1
        assert (k_.value, ko_.value, t_.value) == (K, Ko, T)
        k_.value = ko_.value = t_.value = 0
        assert dl(h, None, None, None, None, None, None, None, 0, short_idx.ctypes.data, T - 1, C.byref(k_), C.byref(ko_), C.byref(t_)) == 1
        assert (k_.value, ko_.value, t_.value) == (K, Ko, T)
        assert dl(h, None, None, None, None, None, None, None, 0, None, 0, C.byref(k_), C.byref(ko_), C.byref(t_)) == 0   # the sizing call
        assert (k_.value, ko_.value, t_.value) == (K, Ko, T)
        parts = [c.slab_partner_problem_download() for c in grp]
        assert len(parts[r]["ids"]) == K and parts[r]["n_owned"] == Ko and len(parts[r]["indices"]) == T
        # a later sph_slab_candidates_prepare replaces the rows: the problem is dropped, the rows are there
        ffi.group_slab_candidates_prepare(grp, "merge", p, ap)
        refused(1, grp[r].slab_partner_problem_download)
        grp[r].slab_candidates_download()
        # the apply's argument refusals: nothing on the device is written
        pids, *fields, off_c, idx_c = D.merge_slab_partner_problems(parts)
        mp_c, mc_c = D._decide_compact(product_lib, "merge", pids, fields, off_c, idx_c, P, dt)
        assert mc_c.sum() > 0 and len(pids) > 2
        swapped = pids.copy()
        swapped[[0, 1]] = swapped[[1, 0]]
        repeated = pids.copy()
        repeated[1] = repeated[0]
        beyond = pids.copy()
        beyond[-1] = n
        outside = mp_c.copy()
        outside[0] = len(pids)
        for op in KINDS:
            refused(1, ffi.group_adapt_compact, grp, op, p, ap, swapped, mp_c, mc_c)     # not ascending
            refused(1, ffi.group_adapt_compact, grp, op, p, ap, repeated, mp_c, mc_c)    # not strictly
            refused(1, ffi.group_adapt_compact, grp, op, p, ap, beyond, mp_c, mc_c)      # an id >= n_global
            refused(1, ffi.group_adapt_compact, grp, op, p, ap, pids, outside, mc_c)     # a partner that is neither a sentinel nor < k
        refused(1, ffi.group_adapt_compact, grp, 2, p, ap, pids, mp_c, mc_c)             # a split takes no decisions
        assert_same_state(state0, state_by_id(grp, n), "refused applies")
        # the state was left able to take the real apply; a renumbering merge drops the problem
        ffi.group_slab_partner_problem_prepare(grp, "merge", p, ap)
        ffi.group_adapt_compact(grp, "merge", p, ap, pids, mp_c, mc_c)
        assert sum(c.n for c in grp) < n
        refused(1, grp[0].slab_partner_problem_download)
        refused(1, ffi.group_slab_partner_problem_prepare, grp, "merge", p, ap)  # the vector was renumbered: no lists until the next step
        sts = ffi.group_step(grp, p)
        for c in grp:
            c.classify(p)
        ap = A.adapt_params(P, float(sts[0].dt))
        ffi.group_slab_partner_problem_prepare(grp, "share", p, ap)
        ffi.group_step(grp, p)
        refused(1, grp[0].slab_partner_problem_download)                         # dropped by the step
        for c in grp:
            c.classify(p)
        ffi.group_slab_partner_problem_prepare(grp, "share", p, ap)
        grp[0].upload_field("mass", grp[0].download("mass"))                     # a mass upload drops this rank's problem
        refused(1, grp[0].slab_partner_problem_download)
        grp[1].slab_partner_problem_download()
        sts = ffi.group_step(grp, p)
        for c in grp:
            c.classify(p)
        ffi.group_slab_partner_problem_prepare(grp, "share", p, ap)
        pid0 = grp[0].download("particle_id")
        grp[0].apply_edits([])                                                   # an edit call, even an empty one, is an edit
        refused(1, grp[0].slab_partner_problem_download)
        assert np.array_equal(np.sort(pid0), np.sort(grp[0].download("particle_id")))
    finally:
        plain.close()
        close_all(grp)


def test_a_poisoned_group_and_an_upload(product_lib):
    """A group poisoned by a step that ran out of room (tests/test_gpu_slab_candidates.py) answers SPH_ERR_POISONED from every entry
    point; behind the re-upload nothing is prepared (no step yet), and behind two steps the problem is there again."""
    scn = sc.dam_break_small(96, 48, 1 / 48)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    P = dam_break_params(max_iters=3, level_estimation_method="EmptyAngle", maximum_surface_distance=0.2, particle_radius_fine=0.004,
                         particle_radius_base=0.02)
    p = P.to_ffi()
    ap = A.adapt_params(P, 1e-3)
    cuts = D.slab_cuts(pos[:, 0], 2)
    parts = D.partition(pos[:, 0], cuts)
    none = (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint16))
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
        refused(31, ffi.group_slab_partner_problem_prepare, grp, "share", p, ap)
        refused(31, ffi.group_adapt_compact, grp, "share", p, ap, *none)
        for c in grp:
            refused(31, c.slab_partner_problem_prepare, "merge", p, ap)     # (the per-rank entry points answer before they ask for a transport)
            refused(31, c.slab_partner_problem_download)
            refused(31, c.slab_share_particles_compact, p, ap, *none)
            refused(31, c.slab_merge_particles_compact, p, ap, *none)
        low = pos[:, 1] < np.median(pos[:, 1])
        ids = np.cumsum(low) - 1
        for r, c in enumerate(grp):
            mine = parts[r][low[parts[r]]]
            c.upload(mass[mine], pos[mine], vel[mine])
            c.upload_field("particle_id", ids[mine].astype(np.uint32))
        refused(1, ffi.group_slab_partner_problem_prepare, grp, "share", p, ap)   # no longer poisoned: no step yet
        refused(1, grp[0].slab_partner_problem_download)
        for _ in range(2):
            sts = ffi.group_step(grp, p)
        for c in grp:
            c.classify(p)
        counts = ffi.group_slab_partner_problem_prepare(grp, "merge", p, A.adapt_params(P, float(sts[0].dt)))
        for c, (K, Ko, T) in zip(grp, counts):
            q = c.slab_partner_problem_download()
            assert (len(q["ids"]), q["n_owned"], len(q["indices"])) == (K, Ko, T)
    finally:
        close_all(grp)
