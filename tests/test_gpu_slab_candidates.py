"""The candidate export of a slab context (include/sph_slab_candidates.h): the ranks' filtered rows, assembled by global id, against
the host filter adaptivity.partner_candidates_reference applied to the ranks' own full lists and fields, entry by entry; the on-slab
adaptive step in export="candidates" mode against the default (same partner arrays after every pass, bit-identical states), on the
loopback group and with every rank on a thread of its own; sph_slab_sum_mass; the refusals; a split that one rank has no room for
ends the apply on every rank within the call."""
import ctypes as C
import time
from concurrent.futures import ThreadPoolExecutor
from contextlib import nullcontext
from pathlib import Path

import numpy as np
import pytest

from adaptive_sph_amd import adaptivity as A, distributed as D, ffi, scene as sc
from adaptive_sph_amd.workloads import dam_break_params, default_params
from tests.test_gpu_adaptivity import _fields_by_id
from tests.test_gpu_incremental_sort import two_sizes_scene

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
PATTERNS = REPO / "tests" / "golden" / "split-patterns.yaml"
ALLOW = ["allow_share_with_optimal_particle", "allow_share_with_too_small_particle", "allow_merge_with_optimal_particle",
         "allow_merge_on_size_difference"]
DECISION_FIELDS = ("particle_size_class", "mass", "level_estimation", "position", "h2")
KINDS = ("share", "merge")
RADII = dict(particle_radius_fine=0.012, particle_radius_base=0.05, maximum_surface_distance=0.3)   # donors of both kinds from the first step on
T_VALUES = (1, 2, 3, 4, 6)


def default_scene(P):
    scn = sc.SceneConfig.from_yaml(str(REPO / "tests" / "golden" / "default-scene.yaml"))
    pos, mass, vel = sc.init_particles(scn)
    return pos, mass, vel, sc.boundary_planes(scn.boundary, P.init_boundary_handler)


def split_patterns():
    return A.SplitPatterns.load_from_file(PATTERNS)


def close_all(ctxs):
    for c in ctxs:
        c.close()


def gathered(grp, n, p, classify=True):
    if classify:
        for c in grp:
            c.classify(p)
    return {f: D.gather_by_id(grp, f, n) for f in DECISION_FIELDS}


def full_lists(grp):
    ids = [c.download("particle_id") for c in grp]
    n = int(sum(len(i) for i in ids))
    off, idx = D.assemble_lists(ids, [c.download_neighbors() for c in grp], n)
    return ids, n, (off.astype(np.uint32), idx)


def donor_median_x(lib, P, scene, t, policy):
    """The same steps on a plain context: t steps with the adaptive half behind the first t - 1, classified; the median x of the
    donors (of either kind) whose candidate rows are not empty."""
    pos, mass, vel, planes = scene
    g = ffi.Context(lib, 120000, planes)
    try:
        if policy is not None:
            g.set_math_policy(policy)
        g.upload(mass, pos, vel)
        drv = A.AdaptivityDriver(g, split_patterns())
        p = P.to_ffi()
        for s in range(1, t + 1):
            st = g.step(p)
            if s < t:
                drv.single_step_adaptivity(P, float(st.dt), int(st.step_number))
        g.classify(p)
        ap = A.adapt_params(P, float(st.dt))
        x = g.download("position")[:, 0]
        donors = np.zeros(g.n, bool)
        for kind in KINDS:
            off, _ = g.download_partner_candidates(kind, p, ap)
            donors |= np.diff(off.astype(np.int64)) > 0
        assert donors.any(), (t, "no donor with a candidate on the plain context")
        return float(np.median(x[donors])), np.sort(x)
    finally:
        g.close()


def cut_group(lib, scene, P, p, k, cut, xs_sorted, policy):
    """Two loopback ranks cut at `cut`, stepped once; a cut the group refuses as narrower than two ghost layers moves to the nearest x
    it accepts (quantiles of x, outwards from the wanted one).  -> (group, stats of the first step, the cut taken)."""
    pos, mass, vel, planes = scene
    q0 = float(np.searchsorted(xs_sorted, cut)) / len(xs_sorted)
    tries = [cut] + [float(np.quantile(xs_sorted, min(max(q0 + s * d, 0.05), 0.95))) for d in (0.05, 0.1, 0.15, 0.2, 0.3, 0.4) for s in (1, -1)]
    last = None
    for x in tries:
        grp = D.make_loopback_group(lib, pos, mass, vel, planes, k, cuts=[-D.INF, x, D.INF])
        try:
            for c in grp:
                if policy is not None:
                    c.set_math_policy(policy)
                c.set_split_patterns(split_patterns().patterns)
            return grp, ffi.group_step(grp, p), x
        except ffi.SphError as e:
            close_all(grp)
            last = e
            if e.status != 30:
                raise
    raise last


def compare_rows(lib, grp, P, p, dt, kind, ids, n, lists, f, label):
    """Both settings of the four allow_* flags on the group's current state.  -> entries that name a particle of another rank."""
    owner = np.empty(n, np.int64)
    for r, i in enumerate(ids):
        owner[i] = r
    cross = kept = 0
    for allow in (False, True):
        Pa = P.replace(**{a: allow for a in ALLOW})
        counts = ffi.group_slab_candidates_prepare(grp, kind, p, A.adapt_params(Pa, dt))
        rows = [c.slab_candidates_download() for c in grp]
        for c, (n_rows, n_idx), (off, idx) in zip(grp, counts, rows):
            assert off.dtype == np.uint32 and idx.dtype == np.uint32
            assert n_rows == c.n == len(off) - 1 and n_idx == len(idx) == int(off[-1]) and off[0] == 0, (label, kind)
        got_off, got_idx = D.assemble_lists(ids, rows, n)
        ref_off, ref_idx = A.partner_candidates_reference(kind, f["particle_size_class"], f["mass"], f["position"], f["h2"], lists[0], lists[1], Pa)
        assert np.array_equal(got_off, ref_off.astype(np.int64)), (label, kind, allow)
        assert np.array_equal(got_idx, ref_idx), (label, kind, allow)
        cross += sum(int((owner[idx] != r).sum()) for r, (_, idx) in enumerate(rows))
        kept += len(got_idx)
    print(f"{label} {kind}: n={n} list entries={len(lists[1])} candidates (allow off + on)={kept}, of another rank={cross}")
    return cross, kept


@pytest.mark.parametrize("policy,after", [("fast", False), ("exact", False), ("fast", True)])
def test_rows_equal_the_numpy_contract(product_lib, policy, after):
    """Two loopback ranks of configs[0], cut at the median x of the donors with candidates: at the adaptive steps t the share rows
    behind the step and the merge rows behind the applied share equal partner_candidates_reference on the gathered fields and the
    ranks' assembled sph_download_neighbors rows (downloaded before the share), under both settings of the four allow_* flags.  For
    each kind some entry must name a particle the OTHER rank owns: without one no ghost's record or class was read.  `after`:
    level_estimation_after_advection -- the rows are then filtered from the extended lists of the advected positions."""
    P = default_params(level_estimation_after_advection=after)
    scene = default_scene(P)
    p = P.to_ffi()
    cross = {k: 0 for k in KINDS}
    kept = {k: 0 for k in KINDS}
    for t in T_VALUES:
        cut, xs = donor_median_x(product_lib, P, scene, t, policy)
        grp, sts, cut_taken = cut_group(product_lib, scene, P, p, 2, cut, xs, policy)
        try:
            for s in range(1, t + 1):
                if s > 1:
                    sts = ffi.group_step(grp, p)
                dt, num = float(sts[0].dt), int(sts[0].step_number)
                if s < t:
                    D.group_single_step_adaptivity_on_slabs(product_lib, grp, P, dt, num)
            ap = A.adapt_params(P, dt)
            ids, n, lists = full_lists(grp)
            label = f"t={t} [{policy}, after={after}] cut {cut_taken:.4f} (wanted {cut:.4f})"
            f = gathered(grp, n, p)
            c, k = compare_rows(product_lib, grp, P, p, dt, "share", ids, n, lists, f, label)
            cross["share"] += c
            kept["share"] += k
            mp, mc = D._decide_on_gathered(product_lib, "share", f, lists, P, dt)
            ffi.group_adapt(grp, "share", p, ap, mp, mc)
            f = gathered(grp, n, p)                    # the fields behind the share, the lists of the step
            c, k = compare_rows(product_lib, grp, P, p, dt, "merge", ids, n, lists, f, label + f" behind {int(mc.sum())} shares")
            cross["merge"] += c
            kept["merge"] += k
            ffi.group_step(grp, p)                     # the export left the group able to step
        finally:
            close_all(grp)
    assert all(v > 0 for v in kept.values()), kept
    assert all(v > 0 for v in cross.values()), cross


def test_three_ranks_with_ghosts_on_both_sides(product_lib):
    """The same comparison where the middle rank has a ghost layer on either side: the two-size scene of the sort tests on three
    ranks.  Entries that name another rank's particle must occur across BOTH cuts."""
    scn = two_sizes_scene()
    pos, mass, vel = sc.init_particles(scn)
    r_fine = float(np.sqrt(np.float32(0.02) ** 2 * 0.93 / np.pi))
    P = dam_break_params(level_estimation_method="EmptyAngle", particle_radius_fine=r_fine, particle_radius_base=4 * r_fine, maximum_surface_distance=0.3,
                         max_iters=6)
    planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    p = P.to_ffi()
    # equal counts put both cuts into the fine block and leave the middle rank narrower than its two ghost layers.  The right cut goes
    # to the interface of the blocks (x = -0.39: that is where a donor's candidates are of the other size; inside the coarse block no
    # row keeps an entry), its layer is 4 coarse h = 0.33 wide; the left cut where only fine particles are in reach (a layer of 0.083)
    # and the middle rank still holds both layers: x <= -0.80.  The first pair the group accepts.
    grp, last = None, None
    for c1, c2 in [(a, b) for b in (-0.39, -0.40, -0.38) for a in (-0.83, -0.85, -0.82, -0.87)]:
        grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 3, cuts=[-D.INF, c1, c2, D.INF])
        try:
            sts = ffi.group_step(grp, p)
            print(f"three ranks: cuts {c1}, {c2}")
            break
        except ffi.SphError as e:
            close_all(grp)
            grp, last = None, e
            if e.status != 30:
                raise
    if grp is None:
        raise last
    try:
        for _ in range(2):
            sts = ffi.group_step(grp, p)
        dt = float(sts[0].dt)
        ids, n, lists = full_lists(grp)
        owner = np.empty(n, np.int64)
        for r, i in enumerate(ids):
            owner[i] = r
        f = gathered(grp, n, p)
        print("three ranks: owned", [c.n for c in grp], "classes", np.bincount(f["particle_size_class"], minlength=5).tolist())
        across = {(0, 1): 0, (1, 2): 0}
        kept = {k: 0 for k in KINDS}
        for kind in KINDS:
            for allow in (False, True):
                Pa = P.replace(**{a: allow for a in ALLOW})
                ffi.group_slab_candidates_prepare(grp, kind, p, A.adapt_params(Pa, dt))
                rows = [c.slab_candidates_download() for c in grp]
                got_off, got_idx = D.assemble_lists(ids, rows, n)
                ref_off, ref_idx = A.partner_candidates_reference(kind, f["particle_size_class"], f["mass"], f["position"], f["h2"], lists[0], lists[1], Pa)
                assert np.array_equal(got_off, ref_off.astype(np.int64)) and np.array_equal(got_idx, ref_idx), (kind, allow)
                kept[kind] += len(ref_idx)
                for r, (_, idx) in enumerate(rows):
                    for o in np.unique(owner[idx]):
                        if o != r:
                            assert abs(int(o) - r) == 1
                            across[(min(r, int(o)), max(r, int(o)))] += int((owner[idx] == o).sum())
        print("three ranks: candidates", kept, "entries of another rank across the cuts", across)
        assert all(v > 0 for v in kept.values()), kept
        assert all(v > 0 for v in across.values()), across
        ffi.group_step(grp, p)
    finally:
        close_all(grp)


class _Threads:
    """k ranks on k threads: the per-rank entry points called the way the ranks of a multi-process run call them."""

    def __init__(self, grp):
        self.grp = grp
        self.pool = ThreadPoolExecutor(len(grp))

    def all(self, fn):
        return [f.result() for f in [self.pool.submit(fn, c) for c in self.grp]]

    def close(self):
        self.pool.shutdown(wait=True)


def adapt_on_threads(lib, th, P, dt, num, export, passes):
    """single_step_adaptivity on the slabs of a ThreadedGroup: the decisions once, here; every collective from k threads."""
    b = th.grp
    p, ap = P.to_ffi(), A.adapt_params(P, dt)
    ids = [c.download("particle_id") for c in b]
    n = int(sum(len(i) for i in ids))
    lists = None
    if export == "lists":
        off, idx = D.assemble_lists(ids, [c.download_neighbors() for c in b], n)
        lists = (off.astype(np.uint32), idx)
    info = {"shares": 0, "merges": 0, "splits": 0}

    def decide(kind):
        th.all(lambda c: c.classify(p))
        f = {k: D.gather_by_id(b, k, n) for k in DECISION_FIELDS}
        rows = lists
        if export == "candidates":
            th.all(lambda c: c.slab_candidates_prepare(kind, p, ap))
            off, idx = D.assemble_lists(ids, [c.slab_candidates_download() for c in b], n)
            rows = (off.astype(np.uint32), idx)
        mp, mc = D._decide_on_gathered(lib, kind, f, rows, P, dt)
        passes.append((kind, mp.copy(), mc.copy()))
        return mp, mc

    if P.sharing:
        mp, mc = decide("share")
        info["shares"] = int(mc.sum())
        th.all(lambda c: c.share_particles(p, ap, mp, mc))
    if num % 2 == 0:
        mp, mc = decide("merge")
        info["merges"] = int(mc.sum())
        th.all(lambda c: c.merge_particles(p, ap, mp, mc))
    else:
        th.all(lambda c: c.classify(p))
        th.all(lambda c: c.split_particles(p, ap))
        info["splits"] = int(sum(c.n for c in b)) - n
    return info


@pytest.mark.parametrize("transport", ["loopback", "threads"])
def test_same_decisions_same_state(product_lib, monkeypatch, transport):
    """Twin groups in lockstep (the default mode behind the steps before t); at adaptive step t one twin exports candidates, the other
    its lists: merge_partner / merge_counter of every pass are identical, and so is every field by id afterwards.  On the threads
    transport every rank enters sph_slab_candidates_prepare from its own thread, like sph_share_particles."""
    P = default_params()
    pos, mass, vel, planes = default_scene(P)
    p = P.to_ffi()
    k = 2
    seen = {"shares": 0, "merges": 0, "splits": 0}
    passes = {"lists": [], "candidates": []}
    current = [None]
    inner = D._decide_on_gathered

    def recording(lib, kind, g, lists, P_, dt_):
        mp, mc = inner(lib, kind, g, lists, P_, dt_)
        if current[0] is not None:
            passes[current[0]].append((kind, mp.copy(), mc.copy()))
        return mp, mc

    if transport == "loopback":
        monkeypatch.setattr(D, "_decide_on_gathered", recording)
    for t in T_VALUES:
        twins, closers = {}, []
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
            info = {}
            for s in range(1, t + 1):
                for mode, (grp, step, th) in twins.items():
                    sts = step(p)
                    dt, num = float(sts[0].dt), int(sts[0].step_number)
                    export = mode if s == t else "lists"
                    current[0] = mode if s == t else None
                    if th is None:
                        info[mode] = D.group_single_step_adaptivity_on_slabs(product_lib, grp, P, dt, num, export=export)
                        if s == t:
                            assert info[mode]["export"] == mode
                    else:
                        info[mode] = adapt_on_threads(product_lib, th, P, dt, num, export, passes[mode] if s == t else [])
                    current[0] = None
            la, ca = passes["lists"], passes["candidates"]
            assert len(la) == len(ca) > 0, (t, len(la), len(ca))
            for (k1, mp1, mc1), (k2, mp2, mc2) in zip(la, ca):
                assert k1 == k2 and np.array_equal(mp1, mp2) and np.array_equal(mc1, mc2), (t, k1)
            la.clear()
            ca.clear()
            for key in seen:
                assert info["lists"][key] == info["candidates"][key], (t, key)
                seen[key] += info["candidates"][key]
            if transport == "loopback":
                print(f"t={t}: exported indices lists {info['lists']['exported_indices']} / candidates {info['candidates']['exported_indices']}, "
                      f"bytes down {info['lists']['bytes_down']} / {info['candidates']['bytes_down']}")
                assert info["candidates"]["exported_indices"] < info["lists"]["exported_indices"]
            n = sum(c.n for c in twins["lists"][0])
            assert n == sum(c.n for c in twins["candidates"][0])
            fa, fb = _fields_by_id(twins["lists"][0], n), _fields_by_id(twins["candidates"][0], n)
            for f in fa:
                assert np.array_equal(fa[f].view(np.uint8), fb[f].view(np.uint8)), (t, f)
            for grp, step, th in twins.values():
                step(p)
        finally:
            for f in reversed(closers):
                f()
    assert all(v > 0 for v in seen.values()), seen


AMPLE = 70000


def slab_ranks(lib, scene, cuts, capacities, group=None):
    """The ranks of `cuts` with split patterns loaded, rank r with room for capacities[r] particles; on the thread transport of `group`
    or, without one, for the loopback entry points."""
    pos, mass, vel, planes = scene
    parts = D.partition(pos[:, 0], cuts)
    k = len(parts)
    ctxs = []
    for r, sel in enumerate(parts):
        c = ffi.Context(lib, capacities[r], planes)
        ctxs.append(c)
        c.dist_configure(r, k, cuts[r], cuts[r + 1])
        if group is not None:
            c.comm_init_threads(group, r, k)
        c.upload(mass[sel], pos[sel], vel[sel])
        c.upload_field("particle_id", sel.astype(np.uint32))
        c.set_split_patterns(split_patterns().patterns)
    return ctxs


def split_probe(lib, P, scene, cuts):
    """A loopback group with ample capacity, stepped and adapted until an adaptive step splits.  -> (that step t, the ranks' owned
    particles in front of the split, their children, the children's x)."""
    p = P.to_ffi()
    grp = slab_ranks(lib, scene, cuts, [AMPLE] * (len(cuts) - 1))
    try:
        for t in range(1, 8):
            sts = ffi.group_step(grp, p)
            owned = [c.n for c in grp]
            ghosts = [sum(c.dist_get_stats()["n_ghost"]) for c in grp]
            info = D.group_single_step_adaptivity_on_slabs(lib, grp, P, float(sts[0].dt), int(sts[0].step_number))
            if info["splits"]:
                children = [c.n - o for c, o in zip(grp, owned)]
                x = np.concatenate([c.download("position")[c.download("particle_id") >= sum(owned), 0] for c in grp])
                print(f"split probe: cuts {cuts[1:-1]} step {t}: owned {owned} ghosts {ghosts} children {children}")
                assert len(x) == info["splits"] == sum(children)
                return t, owned, children, x
        raise AssertionError("no adaptive step of the first seven splits")
    finally:
        close_all(grp)


class _RankStatuses(_Threads):
    """... and what every rank's call returned, and how long the ranks took together, when one of them fails."""

    def all(self, fn):
        t0 = time.perf_counter()
        futs = [self.pool.submit(fn, c) for c in self.grp]
        self.statuses, out, err = [], [], None
        for f in futs:
            try:
                out.append(f.result())
                self.statuses.append(0)
            except ffi.SphError as e:
                self.statuses.append(e.status)
                err = err or e
        self.wall = time.perf_counter() - t0
        if err:
            raise err
        return out


@pytest.mark.parametrize("transport", ["loopback", "threads"])
def test_a_split_without_room_on_one_rank_fails_on_every_rank(product_lib, transport):
    """The collective rule on the adapt path.  Two ranks of the default scene; a probe group with ample capacity tells the adaptive
    step that splits and rank 1's owned particles and children there (at least one child: the cut moves to the children's median x
    if the equal-count cut leaves rank 1 none).  The same run with rank 1's capacity one short of owned + children: the split is
    refused on the host before rank 1's apply kernel is launched -- SPH_ERR_CAPACITY there, and a non-zero status on every rank within
    the same call, whether the group enters through sph_group_adapt or every rank through sph_split_particles on its own thread
    (nobody waits in a collective for the rank that left: the wall time is bounded as in
    test_ranks_on_threads_capacity_failure_is_collective)."""
    P = default_params()
    scene = default_scene(P)
    p = P.to_ffi()
    k = 2
    cuts = D.slab_cuts(scene[0][:, 0], k)
    t, owned, children, x = split_probe(product_lib, P, scene, cuts)
    if children[1] == 0:
        cuts = [-D.INF, float(np.median(x)), D.INF]
        t, owned, children, x = split_probe(product_lib, P, scene, cuts)
    assert children[1] > 0, (cuts, owned, children)
    caps = [AMPLE, owned[1] + children[1] - 1]
    group = C.c_void_p()
    if transport == "threads":
        assert product_lib.thread_group_create(k, C.byref(group)) == 0
    grp = slab_ranks(product_lib, scene, cuts, caps, group if transport == "threads" else None)
    th = _RankStatuses(grp) if transport == "threads" else None
    try:
        for s in range(1, t + 1):
            sts = th.all(lambda c: c.step(p)) if th else ffi.group_step(grp, p)
            dt, num = float(sts[0].dt), int(sts[0].step_number)
            if s == t:
                assert [c.n for c in grp] == owned
            with pytest.raises(ffi.SphError) if s == t else nullcontext() as e:
                if th:
                    adapt_on_threads(product_lib, th, P, dt, num, "lists", [])
                else:
                    D.group_single_step_adaptivity_on_slabs(product_lib, grp, P, dt, num)
        print(f"split without room [{transport}]: capacities {caps}, status {e.value.status}" + (f", per rank {th.statuses} in {th.wall:.3f} s" if th else "") +
              f": {e.value}")
        if th:
            assert th.wall < 30.0
            assert th.statuses[1] == 3 and all(st != 0 for st in th.statuses), th.statuses   # SPH_ERR_CAPACITY on rank 1, its status on the other
        else:
            assert e.value.status == 3 and "on rank 1" in str(e.value), e.value
        assert grp[1].n == owned[1]                                                             # refused before anything of rank 1 was regathered
    finally:
        if th:
            th.close()
        close_all(grp)
        if group:
            product_lib.thread_group_destroy(group)


def test_the_export_writes_nothing(product_lib):
    """step -> prepare + download of both kinds -> step against step -> step: every field by id, bit for bit."""
    P = default_params()
    pos, mass, vel, planes = default_scene(P)
    p = P.to_ffi()
    a = D.make_loopback_group(product_lib, pos, mass, vel, planes, 2)
    b = D.make_loopback_group(product_lib, pos, mass, vel, planes, 2)
    try:
        for grp in (a, b):
            for _ in range(2):
                sts = ffi.group_step(grp, p)
            for c in grp:
                c.classify(p)
        n = len(mass)
        ap = A.adapt_params(P, float(sts[0].dt))
        before = _fields_by_id(a, n)
        got = 0
        for kind in KINDS:
            ffi.group_slab_candidates_prepare(a, kind, p, ap)
            got += sum(len(c.slab_candidates_download()[1]) for c in a)
        assert got > 0
        after = _fields_by_id(a, n)
        for f in before:
            assert np.array_equal(before[f].view(np.uint8), after[f].view(np.uint8)), f
        for grp in (a, b):
            ffi.group_step(grp, p)
        fa, fb = _fields_by_id(a, n), _fields_by_id(b, n)
        for f in fa:
            assert np.array_equal(fa[f].view(np.uint8), fb[f].view(np.uint8)), f
        for f in ("density", "pressure", "neighbor_count"):
            assert np.array_equal(D.gather_by_id(a, f, n).view(np.uint8), D.gather_by_id(b, f, n).view(np.uint8)), f
    finally:
        close_all(a + b)


def test_slab_sum_mass(product_lib):
    """Per rank against numpy's f64 sum of the downloaded masses to 1e-12 relative (about 10^3 positive addends, each addition within
    2^-53: any two orders agree to 2 n 2^-53 < 3e-13); two calls on equal state give equal bits; before a step (no ownership flags
    yet) and behind one (ghosts in the arrays); the ranks' total passes the driver's 0.005 check across an adaptive step."""
    P = default_params()
    pos, mass, vel, planes = default_scene(P)
    p = P.to_ffi()
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 2)
    try:
        for c in grp:
            c.set_split_patterns(split_patterns().patterns)

        def check():
            tot = 0.0
            for c in grp:
                d1, d2 = c.slab_sum_mass(), c.slab_sum_mass()
                assert np.float64(d1).tobytes() == np.float64(d2).tobytes()
                ref = float(np.sum(c.download("mass"), dtype=np.float64))
                print(f"slab_sum_mass rank {grp.index(c)}: n={c.n} device={d1!r} numpy={ref!r} relative {abs(d1 - ref) / ref:.3e}")
                assert abs(d1 - ref) <= 1e-12 * ref
                tot += d1
            return tot

        m0 = check()
        assert abs(m0 - float(np.sum(mass, dtype=np.float64))) <= 1e-12 * m0
        events = 0
        for _ in range(2):
            sts = ffi.group_step(grp, p)
            assert sum(sum(c.dist_get_stats()["n_ghost"]) for c in grp) > 0
            m1 = check()
            info = D.group_single_step_adaptivity_on_slabs(product_lib, grp, P, float(sts[0].dt), int(sts[0].step_number), export="candidates")
            events += info["shares"] + info["merges"] + info["splits"]
            m2 = check()
            assert abs(m1 - m2) <= 0.005
        assert events > 0
        ffi.group_step(grp, p)
    finally:
        close_all(grp)


def test_refusals(product_lib):
    P = default_params(**RADII)
    pos, mass, vel, planes = default_scene(P)
    p = P.to_ffi()
    ap = A.adapt_params(P, 1e-3)

    def refused(status, f, *a):
        with pytest.raises(ffi.SphError) as e:
            f(*a)
        assert e.value.status == status, e.value

    plain = ffi.Context(product_lib, 70000, planes)
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 2)
    try:
        plain.upload(mass, pos, vel)
        plain.step(p)
        refused(30, plain.slab_candidates_prepare, "share", p, ap)           # a plain context
        refused(30, plain.slab_candidates_download)
        refused(30, plain.slab_sum_mass)
        refused(1, ffi.group_slab_candidates_prepare, grp, "share", p, ap)   # no step before
        refused(1, grp[0].slab_candidates_download)                          # nothing prepared
        sts = ffi.group_step(grp, p)
        dt = float(sts[0].dt)
        ap = A.adapt_params(P, dt)
        for c in grp:
            c.classify(p)
        refused(1, ffi.group_slab_candidates_prepare, grp, 2, p, ap)         # kind
        refused(1, ffi.group_slab_candidates_prepare, grp, "merge", None, ap)  # null params
        refused(1, ffi.group_slab_candidates_prepare, grp, "merge", p, None)
        refused(1, grp[0].slab_candidates_download)                          # the refusals prepared nothing
        counts = ffi.group_slab_candidates_prepare(grp, "merge", p, ap)
        r = max(range(2), key=lambda i: counts[i][1])
        n_rows, n_idx = counts[r]
        assert n_idx > 1
        short = np.empty(n_idx - 1, np.uint32)
        rc = product_lib.slab_candidates_download(grp[r].handle, None, short.ctypes.data, short.size)
        assert rc == 1                                                       # capacity one short
        off, idx = grp[r].slab_candidates_download()
        assert len(off) == n_rows + 1 and len(idx) == n_idx == off[-1]
        ffi.group_step(grp, p)
        refused(1, grp[r].slab_candidates_download)                          # dropped by the step
        # prepare(merge) behind a share with no CSR built before it: the share's apply took the snapshot the lists are rebuilt from
        ids, n, lists = full_lists(grp)
        f = gathered(grp, n, p)
        mp, mc = D._decide_on_gathered(product_lib, "share", f, lists, P, dt)
        assert mc.sum() > 0
        ffi.group_adapt(grp, "share", p, ap, mp, mc)
        refused(1, ffi.group_slab_candidates_prepare, grp, "merge", p, ap)
        sts = ffi.group_step(grp, p)                                         # ... and the group still steps
        # prepare(merge) behind a merge apply: the vector was renumbered
        ids, n, lists = full_lists(grp)
        f = gathered(grp, n, p)
        counts = ffi.group_slab_candidates_prepare(grp, "merge", p, ap)
        off_c, idx_c = D.assemble_lists(ids, [c.slab_candidates_download() for c in grp], n)
        mp, mc = D._decide_on_gathered(product_lib, "merge", f, (off_c.astype(np.uint32), idx_c), P, float(sts[0].dt))
        assert mc.sum() > 0
        ffi.group_adapt(grp, "merge", p, A.adapt_params(P, float(sts[0].dt)), mp, mc)
        refused(1, ffi.group_slab_candidates_prepare, grp, "merge", p, ap)
        refused(1, grp[0].slab_candidates_download)
        ffi.group_step(grp, p)
        for c in grp:
            c.classify(p)
        ffi.group_slab_candidates_prepare(grp, "share", p, ap)
        grp[0].upload_field("mass", grp[0].download("mass"))                 # a mass upload drops this rank's rows and lists
        refused(1, grp[0].slab_candidates_download)
        grp[1].slab_candidates_download()
        ffi.group_step(grp, p)
    finally:
        plain.close()
        close_all(grp)


def test_a_poisoned_slab_group_is_refused_until_the_upload(product_lib):
    """Contexts with room for their owned particles but not for a ghost layer: the step ends in SPH_ERR_CAPACITY on every rank and
    leaves them poisoned (test_a_slab_without_room_for_its_ghosts_says_so).  Every entry point then answers SPH_ERR_POISONED; behind a
    re-upload -- of the lower half of the column, which fits with its ghosts -- the group steps and exports again."""
    scn = sc.dam_break_small(96, 48, 1 / 48)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    P = dam_break_params(max_iters=3, level_estimation_method="EmptyAngle", maximum_surface_distance=0.2, particle_radius_fine=0.004,
                         particle_radius_base=0.02)
    p = P.to_ffi()
    ap = A.adapt_params(P, 1e-3)
    cuts = D.slab_cuts(pos[:, 0], 2)
    parts = D.partition(pos[:, 0], cuts)

    def refused(status, f, *a):
        with pytest.raises(ffi.SphError) as e:
            f(*a)
        assert e.value.status == status, e.value

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
        with pytest.raises(ffi.SphError):
            ffi.group_step(grp, p)                                           # poisoned until sph_upload
        refused(31, ffi.group_slab_candidates_prepare, grp, "share", p, ap)
        for c in grp:
            refused(31, c.slab_candidates_prepare, "merge", p, ap)          # (the per-rank entry point answers before it asks for a transport)
            refused(31, c.slab_candidates_download)
            refused(31, c.slab_sum_mass)
        low = pos[:, 1] < np.median(pos[:, 1])
        ids = np.cumsum(low) - 1
        for r, c in enumerate(grp):
            mine = parts[r][low[parts[r]]]
            assert 0 < 2 * len(mine) <= len(parts[r]) + 8
            c.upload(mass[mine], pos[mine], vel[mine])
            c.upload_field("particle_id", ids[mine].astype(np.uint32))
        m = sum(c.slab_sum_mass() for c in grp)
        assert abs(m - float(np.sum(mass[low], dtype=np.float64))) <= 1e-12 * m
        refused(1, ffi.group_slab_candidates_prepare, grp, "share", p, ap)   # no longer poisoned: no step yet
        for _ in range(2):
            sts = ffi.group_step(grp, p)
        for c in grp:
            c.classify(p)
        counts = ffi.group_slab_candidates_prepare(grp, "merge", p, A.adapt_params(P, float(sts[0].dt)))
        for c, (n_rows, n_idx) in zip(grp, counts):
            off, idx = c.slab_candidates_download()
            assert n_rows == c.n == len(off) - 1 and n_idx == len(idx)
    finally:
        close_all(grp)
