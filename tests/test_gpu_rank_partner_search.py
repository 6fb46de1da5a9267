"""The partner searches on the device with one rank per host thread, each calling for itself over the thread transport
(include/sph_rank_partner_search.h): the problem merged on the root behind the relay against distributed.merge_slab_partner_problems on
the ranks' downloaded local problems, bit for bit; every rank's decisions against the sequential loop on that problem; the relay's byte
counts against sph_relay_plan; the apply and whole adaptive steps against the per-rank "compact" mode and against the in-process group
form; the refusals and the solution's lifetime; an empty relay on a one-rank RCCL communicator.

Scenes and radii are those of tests/test_gpu_slab_partner_search.py: the default scene (1 035 particles) on two ranks cut at the donor
median, the two-size scene on three ranks (a two-hop relay through the middle rank; the middle rank as root receives from both sides in
one round), the default scene at half spacing (4 176 particles) where a blob takes several 4 096-byte sub-rounds.

Not tested here: the merge's and the solver's error words (not reachable through a public call), and therefore the header that carries
them to every rank; an apply that fails behind the agreement (the solution is marked consumed in front of the apply)."""
import ctypes as C
import threading
from pathlib import Path

import numpy as np
import pytest
import yaml

from adaptive_sph_amd import adaptivity as A, distributed as D, ffi, scene as sc
from adaptive_sph_amd.workloads import dam_break_params, default_params
from tests.test_gpu_partner_search import NOBODY_LARGE
from tests.test_gpu_slab_candidates import RADII, _Threads, close_all, default_scene, donor_median_x, split_patterns
from tests.test_gpu_slab_partner_problem import PART_KEYS, assert_same_state, compact_on_threads, same_bits, state_by_id, three_rank_setup

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
ALLOW = ("allow_share_with_optimal_particle", "allow_share_with_too_small_particle", "allow_merge_with_optimal_particle", "allow_merge_on_size_difference")
NOBODY_TOO_SMALL = dict(particle_radius_fine=0.001, particle_radius_base=0.002, maximum_surface_distance=0.3)   # every target mass far below every particle's


class Ranks:
    """k slab contexts on the thread transport, every collective entered from k threads; `total`: the sum over the ranks as the rank
    driver wants it where there is no launcher (a barrier between the ranks' threads)."""

    def __init__(self, lib, scene, k, cuts=None, policy=None):
        pos, mass, vel, planes = scene
        self.tg = D.ThreadedGroup(lib, pos, mass, vel, planes, k, cuts=cuts)
        self.grp = self.tg.contexts
        self.k = k
        self.th = _Threads(self.grp)
        self.barrier = threading.Barrier(k)
        self.slots = [0] * k
        for c in self.grp:
            if policy is not None:
                c.set_math_policy(policy)
            c.set_split_patterns(split_patterns().patterns)

    def step(self, p):
        return self.tg.step(p)

    def all(self, fn):
        """fn(context) on every rank's thread; the first error is raised after every rank has returned"""
        out = self.each(fn)
        for v in out:
            if isinstance(v, Exception):
                raise v
        return out

    def each(self, fn):
        def call(c):
            try:
                return fn(c)
            except ffi.SphError as e:
                return e
        return self.th.all(call)

    def refused(self, status, fn, needle=None):
        """every rank takes the same refusal"""
        out = self.each(fn)
        assert all(isinstance(v, ffi.SphError) and v.status == status for v in out), out
        if needle:
            assert all(needle in str(v) for v in out), out

    def total(self, c):
        r = self.grp.index(c)

        def total(v):
            self.slots[r] = v
            self.barrier.wait(timeout=120)
            s = sum(self.slots)
            self.barrier.wait(timeout=120)
            return s
        return total

    def n(self):
        return int(sum(c.n for c in self.grp))

    def close(self):
        self.th.close()
        self.tg.close()


def ranks_that_step(lib, scene, k, p, steps, cut_tries, policy=None):
    """the first cuts of `cut_tries` the ranks accept (a slab narrower than two ghost layers is refused with status 30), `steps` steps
    -> (ranks, the last step's stats, the cuts)"""
    last = None
    for cuts in cut_tries:
        R = Ranks(lib, scene, k, cuts, policy)
        try:
            for _ in range(steps):
                sts = R.step(p)
            return R, sts, cuts
        except ffi.SphError as e:
            R.close()
            last = e
            if e.status != 30:
                raise
    raise last


def two_ranks(lib, P, policy=None):
    """tests/test_gpu_slab_partner_problem.py::two_rank_group on threads: the default scene cut at the donor median, two steps"""
    scene = default_scene(P)
    cut, xs = donor_median_x(lib, P, scene, 1, policy)
    q0 = float(np.searchsorted(xs, cut)) / len(xs)
    tries = [cut] + [float(np.quantile(xs, min(max(q0 + s * d, 0.05), 0.95))) for d in (0.05, 0.1, 0.15, 0.2, 0.3, 0.4) for s in (1, -1)]
    R, sts, _ = ranks_that_step(lib, scene, 2, P.to_ffi(), 2, [[-D.INF, x, D.INF] for x in tries], policy)
    return R, float(sts[0].dt), int(sts[0].step_number)


def three_ranks(lib, P, scene):
    """tests/test_gpu_slab_partner_problem.py::three_rank_group on threads: the two-size scene, three steps"""
    tries = [[-D.INF, a, b, D.INF] for b in (-0.39, -0.40, -0.38) for a in (-0.83, -0.85, -0.82, -0.87)]
    R, sts, _ = ranks_that_step(lib, scene, 3, P.to_ffi(), 3, tries)
    return R, float(sts[0].dt), int(sts[0].step_number)


def half_spacing_scene(P):
    doc = yaml.safe_load((REPO / "tests" / "golden" / "default-scene.yaml").read_text())
    for b in doc["blocks"]:
        b["spacing"] = b["spacing"] * 0.5
    scn = sc.SceneConfig.from_mapping(doc)
    pos, mass, vel = sc.init_particles(scn)
    assert len(mass) == 4176
    return pos, mass, vel, sc.boundary_planes(scn.boundary, P.init_boundary_handler)


def bare(info):
    return {k: v for k, v in info.items() if k != "local"}


def planned_traffic(lib, k, root, rank, sizes):
    """what sph_relay_plan says `rank` sends and receives in the gather and the two broadcasts of one search -> (sent, received, the
    gather's sub-rounds per round)"""
    sent = received = 0
    per_round = {}
    relays = [(sizes["bytes_of_rank"], False)]
    for b in (sizes["header_bytes"], sizes["decisions_bytes"]):
        relays.append(([b if r == root else 0 for r in range(k)], True))
    for i, (blobs, outwards) in enumerate(relays):
        for s in ffi.relay_plan(lib, k, root, rank, blobs, sizes["chunk_bytes"], outwards=outwards):
            sent += s["send"][0][2] + s["send"][1][2]
            received += s["recv"][0][2] + s["recv"][1][2]
            if i == 0:
                per_round[s["round"]] = per_round.get(s["round"], 0) + 1
    return sent, received, per_round


def find_against_the_host(lib, R, P, p, dt, kind, label, root=0, relay_bytes=0, wide_threshold=0):
    """sph_slab_find_partners_device on every rank: the merged problem on the root == the numpy merge of the ranks' downloaded local
    problems, every rank's decisions == the loop's on that problem, the info == the numpy counts and the same on every rank, what the
    relay moved == sph_relay_plan's sums.  -> (merged problem, decisions, info, the ranks' local problems)"""
    ap = A.adapt_params(P, dt)
    R.all(lambda c: c.classify(p))
    infos = R.all(lambda c: c.slab_find_partners_device(kind, p, ap, wide_threshold=wide_threshold, root=root, relay_bytes=relay_bytes))
    parts = [c.slab_partner_problem_download() for c in R.grp]       # the prepare inside the call left them
    assert [i["local"] for i in infos] == [(len(q["ids"]), q["n_owned"], len(q["indices"])) for q in parts], (label, kind)
    assert all(bare(i) == bare(infos[0]) for i in infos), (label, kind, root, infos)
    merged = D.merge_slab_partner_problems(parts)
    got = R.grp[root].slab_download_merged_partner_problem()
    for key, a, b in zip(PART_KEYS, got, merged):
        assert same_bits(a, b), (label, kind, root, key)
    for r, c in enumerate(R.grp):
        if r != root:
            with pytest.raises(ffi.SphError) as e:
                c.slab_download_merged_partner_problem()
            assert e.value.status == 1
    K = len(merged[0])
    pids, *fields, off_c, idx_c = merged
    mp_c, mc_c = D._decide_compact(lib, kind, pids, fields, off_c, idx_c, P, dt) if K else (np.zeros(0, np.uint32), np.zeros(0, np.uint16))
    for r, c in enumerate(R.grp):
        ids, mp, mc = c.slab_download_partner_decisions(K)
        assert np.array_equal(ids, pids), (label, kind, root, r)
        assert np.array_equal(mp, mp_c) and np.array_equal(mc, mc_c), (label, kind, root, r, int(np.count_nonzero(mp != mp_c)))
    want = {"participants": K, "candidates": len(merged[7]), "donors": int(np.count_nonzero(mc_c)), "transfers": int(mc_c.sum())}
    assert {k: infos[0][k] for k in want} == want, (label, kind, root, infos[0])
    sizes = [c.slab_relay_sizes() for c in R.grp]
    assert all({k: v for k, v in s.items() if not k.startswith("bytes_s") and not k.startswith("bytes_rec")} ==
               {k: v for k, v in sizes[0].items() if not k.startswith("bytes_s") and not k.startswith("bytes_rec")} for s in sizes)
    assert sizes[0]["header_bytes"] == (ffi.RANK_HEADER_BYTES if K else 0) and all(b % 16 == 0 for b in sizes[0]["bytes_of_rank"])   # (K == 0: nothing is relayed)
    assert (sizes[0]["decisions_bytes"] > 0) == (K > 0) and [b > 0 for b in sizes[0]["bytes_of_rank"]] == [len(q["ids"]) > 0 for q in parts]
    for r, s in enumerate(sizes):
        sent, received, _ = planned_traffic(lib, R.k, root, r, s)
        assert (s["bytes_sent"], s["bytes_received"]) == (sent, received), (label, kind, root, r)
    assert sum(s["bytes_sent"] for s in sizes) == sum(s["bytes_received"] for s in sizes) and (sizes[0]["bytes_sent"] + sizes[0]["bytes_received"] > 0) == (K > 0)
    print(f"{label} {kind} root={root} relay_bytes={relay_bytes}: {bare(infos[0])} local {[i['local'] for i in infos]} blobs {sizes[0]['bytes_of_rank']} "
          f"decisions {sizes[0]['decisions_bytes']} sent {[s['bytes_sent'] for s in sizes]}")
    return merged, (mp_c.copy(), mc_c.copy()), bare(infos[0]), parts


@pytest.mark.parametrize("policy", ["fast", "exact"])
def test_merge_and_decisions_on_two_ranks(product_lib, policy):
    """The share behind the step with root 0 and root 1, then -- behind the applied share -- the merge with either root."""
    P = default_params()
    p = P.to_ffi()
    R, dt, num = two_ranks(product_lib, P, policy)
    try:
        ap = A.adapt_params(P, dt)
        n = R.n()
        for kind in ("share", "merge"):
            R.all(lambda c: c.classify(p))
            before = state_by_id(R.grp, n)
            found = [find_against_the_host(product_lib, R, P, p, dt, kind, policy, root=root) for root in (0, 1)]
            assert found[0][2] == found[1][2] and found[0][1][1].sum() > 0
            assert all(same_bits(a, b) for a, b in zip(found[0][0], found[1][0]))
            foreign = sum(len(q["ids"]) - q["n_owned"] for q in found[0][3])
            assert foreign > 0, kind
            assert_same_state(before, state_by_id(R.grp, n), f"find + downloads, {kind}")
            if kind == "share":
                R.all(lambda c: c.slab_adapt_device("share", p, ap))
                assert not same_bits(before["mass"], D.gather_by_id(R.grp, "mass", n))
        R.step(p)                                                    # an unused solution leaves the ranks able to step
    finally:
        R.close()


def test_three_ranks_and_every_root(product_lib):
    """Root 0 and root 2: the far rank's blob crosses the middle rank, which forwards in round 2 what it took in round 1.  Root 1: a blob
    from either side in the same round.  The scene exercises the merge: participants only foreign ranks report, and participants two
    ranks report."""
    P, scene = three_rank_setup()
    p = P.to_ffi()
    R, dt, num = three_ranks(product_lib, P, scene)
    try:
        only_foreign = twice = 0
        for kind in ("share", "merge"):
            for allow in (False, True):
                Pa = P.replace(**{a: allow for a in ALLOW})
                found = [find_against_the_host(product_lib, R, Pa, p, dt, kind, f"three ranks allow={allow}", root=root) for root in (0, 1, 2)]
                assert found[0][2] == found[1][2] == found[2][2], (kind, allow)
                for f in found[1:]:
                    assert all(same_bits(a, b) for a, b in zip(found[0][0], f[0])), (kind, allow)
                    assert all(np.array_equal(a, b) for a, b in zip(found[0][1], f[1])), (kind, allow)
                parts = found[0][3]
                owned = np.concatenate([q["ids"][:q["n_owned"]] for q in parts])
                only_foreign += len(np.setdiff1d(found[0][0][0], owned))
                _, counts = np.unique(np.concatenate([q["ids"] for q in parts]), return_counts=True)
                twice += int(np.count_nonzero(counts >= 2))
        print(f"participants reported only as foreign: {only_foreign}, reported by two ranks: {twice}")
        assert only_foreign > 0 and twice > 0, (only_foreign, twice)
        R.step(p)
    finally:
        R.close()


def test_blobs_of_several_sub_rounds(product_lib):
    """The default scene at half spacing on two ranks: n_global and the merge problem's K cross a 2 048-word scan tile, and with
    relay_bytes = 4 096 every blob and the decisions take several sub-rounds.  The same problem, decisions and info as with one message
    per blob."""
    P = default_params(**RADII)
    p = P.to_ffi()
    R = Ranks(product_lib, half_spacing_scene(P), 2)
    try:
        for _ in range(2):
            sts = R.step(p)
        dt = float(sts[0].dt)
        for kind in ("merge", "share"):
            for root in (0, 1):
                whole = find_against_the_host(product_lib, R, P, p, dt, kind, "half spacing", root=root, relay_bytes=0)
                one_message = R.grp[0].slab_relay_sizes()
                cut = find_against_the_host(product_lib, R, P, p, dt, kind, "half spacing", root=root, relay_bytes=4096)
                chunked = R.grp[0].slab_relay_sizes()
                assert whole[2] == cut[2] and all(same_bits(a, b) for a, b in zip(whole[0], cut[0]))
                assert all(np.array_equal(a, b) for a, b in zip(whole[1], cut[1]))
                assert chunked["chunk_bytes"] == 4096 and one_message["chunk_bytes"] > max(one_message["bytes_of_rank"])
                assert chunked["bytes_of_rank"] == one_message["bytes_of_rank"]
                if kind == "merge":                                  # (the share problem of this scene is eight participants on one rank)
                    _, _, per_round = planned_traffic(product_lib, 2, root, 0, chunked)
                    assert per_round and all(v > 1 for v in per_round.values()), per_round
                    assert per_round[1] == -(-chunked["bytes_of_rank"][1 - root] // 4096) > 20
                    assert planned_traffic(product_lib, 2, root, 0, one_message)[2] == {1: 1}
                    assert chunked["decisions_bytes"] > 2 * 4096     # (the broadcast is cut as well)
            if kind == "merge":
                assert len(whole[0][0]) > 2048 and R.n() > 2048 and whole[2]["transfers"] > 0
        R.step(p)
    finally:
        R.close()


def three_rank_twins(lib, P, p):
    """Twin three-rank rows of the default scene at the test radii, one step each.  The scene is two blocks with a gap between them:
    rank 0 takes the coarse block, ranks 1 and 2 share the fine one (equal thirds would cut it into slabs narrower than two ghost
    layers); the first cut through the fine block that the ranks accept."""
    scene = default_scene(P)
    tries = [[-D.INF, 0.0, x, D.INF] for x in (0.675, 0.66, 0.69, 0.645, 0.705)]
    a, sts, cuts = ranks_that_step(lib, scene, 3, p, 1, tries)
    b = Ranks(lib, scene, 3, cuts)
    try:
        b.step(p)
    except Exception:
        a.close()
        b.close()
        raise
    print(f"three ranks: cuts {cuts[1:-1]}, particles {[c.n for c in a.grp]}")
    return a, b, sts, scene


def test_adaptive_steps_equal_the_compact_mode(product_lib):
    """Twin three-rank rows over four adaptive steps -- share + split, share + merge (with deletions), twice --: one takes the per-rank
    "compact" path (local problems down, numpy merge, host loop, decisions up), one the rank driver of the device mode with the middle
    rank as root.  The same events per step and bit-identical states after every step."""
    P = default_params(**RADII)
    p = P.to_ffi()
    a, b, sts, _ = three_rank_twins(product_lib, P, p)
    try:
        seen = {"shares": 0, "merges": 0, "splits": 0}
        for s in range(1, 5):
            if s > 1:
                sts = a.step(p)
                b.step(p)
            dt, num = float(sts[0].dt), int(sts[0].step_number)
            n0 = a.n()
            ia = compact_on_threads(product_lib, a.th, P, dt, num, [])
            ib = b.all(lambda c: D.rank_single_step_adaptivity_on_slabs_device(c, P, dt, num, root=1, total=b.total(c)))
            for key in seen:
                assert all(i[key] == ia[key] for i in ib), (s, key, ia[key], [i[key] for i in ib])
                seen[key] += ia[key]
            n = a.n()
            assert n == b.n() and all(i["n_before"] == n0 and i["n_after"] == n for i in ib)
            assert [c.n for c in a.grp] == [c.n for c in b.grp]
            for i in ib:
                assert i["export"] == "device" and i["bytes_up"] == 0 and i["bytes_down"] == 48 * len(i["passes"]) + 2 * 8
                assert [q["kind"] for q in i["passes"]] == (["share", "merge"] if num % 2 == 0 else ["share"])
                assert all({"participants", "ranks", "rounds", "max_frontier", "wide_rounds"} <= set(q) for q in i["passes"])
                assert i["participants"] == sum(q["participants"] for q in i["passes"])
            assert sum(i["bytes_between_devices"] for i in ib) > 0
            print(f"step {s}: n={n} {ia} passes {[(q['kind'], q['participants'], q['rounds']) for q in ib[1]['passes']]} between devices "
                  f"{[i['bytes_between_devices'] for i in ib]}")
            assert_same_state(state_by_id(a.grp, n), state_by_id(b.grp, n), f"step {s}")
        assert all(v > 0 for v in seen.values()), seen
        a.step(p)
        b.step(p)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("kind", ["share", "merge"])
def test_nobody_to_search_for(product_lib, kind):
    """K == 0: the table says no rank has a donor with a candidate.  No relay, an all-zero info, an open solution without decisions, and
    the apply of it is the compact apply of empty arrays."""
    P = default_params(**RADII)
    p = P.to_ffi()
    Pn = default_params(**(NOBODY_LARGE if kind == "share" else NOBODY_TOO_SMALL))
    pn = Pn.to_ffi()
    a, b, sts, _ = three_rank_twins(product_lib, P, p)
    try:
        apn = A.adapt_params(Pn, float(sts[0].dt))
        for R in (a, b):
            R.all(lambda c: c.classify(pn))
        infos = b.all(lambda c: c.slab_find_partners_device(kind, pn, apn, root=2))
        zero = {"participants": 0, "candidates": 0, "donors": 0, "transfers": 0, "rounds": 0, "max_frontier": 0, "wide_rounds": 0, "local": (0, 0, 0)}
        assert all(i == zero for i in infos), infos
        for c in b.grp:
            assert all(len(v) == 0 for v in c.slab_download_partner_decisions(0))
            s = c.slab_relay_sizes()
            assert s == {"bytes_of_rank": [0, 0, 0], "chunk_bytes": s["chunk_bytes"], "header_bytes": 0, "decisions_bytes": 0, "bytes_sent": 0, "bytes_received": 0}
        assert len(b.grp[2].slab_download_merged_partner_problem()[0]) == 0
        b.all(lambda c: c.slab_adapt_device(kind, pn, apn))
        none = (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint16))
        a.all(lambda c: (c.slab_share_particles_compact if kind == "share" else c.slab_merge_particles_compact)(pn, apn, *none))
        n = a.n()
        assert_same_state(state_by_id(a.grp, n), state_by_id(b.grp, n), kind)
        a.step(p)
        b.step(p)
        assert_same_state(state_by_id(a.grp, n), state_by_id(b.grp, n), kind + " + step")
    finally:
        a.close()
        b.close()


def test_the_state_equals_the_group_forms(product_lib):
    """The same scene and cuts as a loopback group in export="device" (sph_group_find_partners_device, staged by copies) and as ranks
    on threads (staged by the relay): the same merge behind either staging, bit-identical states over two adaptive steps."""
    P = default_params(**RADII)
    p = P.to_ffi()
    scene = default_scene(P)
    pos, mass, vel, planes = scene
    k = 2
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, k)
    R = Ranks(product_lib, scene, k)
    try:
        for c in grp:
            c.set_split_patterns(split_patterns().patterns)
        events = 0
        for s in range(1, 3):
            sts = ffi.group_step(grp, p)
            stt = R.step(p)
            assert float(sts[0].dt) == float(stt[0].dt)
            dt, num = float(sts[0].dt), int(sts[0].step_number)
            ig = D.group_single_step_adaptivity_on_slabs(product_lib, grp, P, dt, num, export="device")
            ir = R.all(lambda c: D.rank_single_step_adaptivity_on_slabs_device(c, P, dt, num, root=s % k, total=R.total(c)))
            for key in ("n_before", "n_after", "shares", "merges", "splits", "participants"):
                assert all(i[key] == ig[key] for i in ir), (s, key)
            events += ig["shares"] + ig["merges"] + ig["splits"]
            assert len(ig["passes"]) == len(ir[0]["passes"])
            for j, q in enumerate(ig["passes"]):
                for key in ("kind", "participants", "rounds", "max_frontier", "wide_rounds"):
                    assert all(i["passes"][j][key] == q[key] for i in ir), (s, j, key)
                assert [tuple(t) for t in q["ranks"]] == [i["passes"][j]["ranks"][0] for i in ir], (s, j)
            n = ig["n_after"]
            assert_same_state(state_by_id(grp, n), state_by_id(R.grp, n), f"step {s}")
        assert events > 0
    finally:
        close_all(grp)
        R.close()


def status_of(f, *args):
    with pytest.raises(ffi.SphError) as e:
        f(*args)
    return e.value.status, str(e.value)


def test_refusals_and_lifetime(product_lib):
    P = default_params(**RADII)
    scene = default_scene(P)
    pos, mass, vel, planes = scene
    p = P.to_ffi()
    ap = A.adapt_params(P, 1e-3)
    plain = ffi.Context(product_lib, 70000, planes)
    loop = D.make_loopback_group(product_lib, pos, mass, vel, planes, 2)
    R = Ranks(product_lib, scene, 2)
    try:
        plain.upload(mass, pos, vel)
        plain.step(p)
        plain.classify(p)
        ffi.group_step(loop, p)
        # a plain context -> UNSUPPORTED, naming the plain entry point; a member of a loopback group -> INVALID_ARGUMENT, naming the group's
        st, msg = status_of(plain.slab_find_partners_device, "share", p, ap)
        assert st == 30 and "sph_find_partners_device" in msg
        assert status_of(plain.slab_adapt_device, "share", p, ap)[0] == 30
        assert status_of(plain.slab_download_partner_decisions, 0)[0] == 30
        assert status_of(plain.slab_download_merged_partner_problem)[0] == 30
        assert status_of(plain.slab_relay_sizes)[0] == 30
        st, msg = status_of(loop[0].slab_find_partners_device, "share", p, ap)
        assert st == 1 and "sph_group_find_partners_device" in msg
        st, msg = status_of(loop[1].slab_adapt_device, "share", p, ap)
        assert st == 1 and "sph_group_adapt_device" in msg
        plain.step(p)
        ffi.group_step(loop, p)
        # no step before the call: the prepare's refusal, on every rank
        R.refused(1, lambda c: c.slab_find_partners_device("share", p, ap))
        sts = R.step(p)
        dt = float(sts[0].dt)
        ap = A.adapt_params(P, dt)
        n = len(mass)
        R.all(lambda c: c.classify(p))
        state0 = state_by_id(R.grp, n)
        R.refused(1, lambda c: c.slab_adapt_device("share", p, ap), "no open solution")          # nothing found yet
        R.refused(1, lambda c: c.slab_download_partner_decisions(0))
        R.refused(1, lambda c: c.slab_download_merged_partner_problem())
        R.refused(1, lambda c: c.slab_relay_sizes())
        R.refused(1, lambda c: c.slab_find_partners_device("share", p, ap, root=2))               # root outside 0 .. nranks-1
        R.refused(1, lambda c: c.slab_find_partners_device("share", p, ap, root=-1))
        R.refused(1, lambda c: c.slab_find_partners_device(2, p, ap))                              # kind
        R.refused(1, lambda c: c.slab_find_partners_device("share", None, ap))
        R.refused(1, lambda c: c.slab_find_partners_device("share", p, None))
        R.refused(1, lambda c: c.slab_find_partners_device("share", p, ap, relay_bytes=4095))     # below 4096
        assert product_lib.slab_find_partners_device(R.grp[0].handle, 0, C.byref(p), C.byref(ap), 0, 0, 0, None, None, None, None) == 1   # info NULL
        R.refused(1, lambda c: c.slab_adapt_device("share", p, ap))                                # the refused calls opened nothing
        assert_same_state(state0, state_by_id(R.grp, n), "refused finds")
        R.step(p)                                                                                  # ... and left the transport usable
        R.all(lambda c: c.classify(p))
        state0 = state_by_id(R.grp, n)
        # an open solution: its kind, its K
        infos = R.all(lambda c: c.slab_find_partners_device("share", p, ap, root=1))
        K = infos[0]["participants"]
        assert K > 0 and infos[0]["transfers"] > 0
        R.refused(1, lambda c: c.slab_adapt_device("merge", p, ap), "of kind 0")                   # a solution of the other kind
        R.refused(1, lambda c: c.slab_adapt_device(2, p, ap))                                      # op
        R.refused(1, lambda c: c.slab_adapt_device("share", None, ap))
        R.refused(1, lambda c: c.slab_adapt_device("share", p, None))
        R.refused(1, lambda c: c.slab_download_partner_decisions(K + 1))                           # k != K
        assert_same_state(state0, state_by_id(R.grp, n), "refused applies")
        sol = [c.slab_download_partner_decisions(K) for c in R.grp]
        assert all(np.array_equal(x, y) for x, y in zip(*sol))
        R.all(lambda c: c.slab_adapt_device("share", p, ap))                                       # the refusals left it open
        assert not same_bits(state0["mass"], D.gather_by_id(R.grp, "mass", n))
        R.refused(1, lambda c: c.slab_adapt_device("share", p, ap))                                # consumed by its own apply
        R.refused(1, lambda c: c.slab_download_partner_decisions(K))
        R.grp[0].slab_partner_problem_download()                                                   # (the share left the prepared problem open)
        # closed by a later prepare
        R.all(lambda c: c.classify(p))
        R.all(lambda c: c.slab_find_partners_device("merge", p, ap))
        R.all(lambda c: c.slab_partner_problem_prepare("merge", p, ap))
        R.refused(1, lambda c: c.slab_adapt_device("merge", p, ap))
        # closed by a step
        infos = R.all(lambda c: c.slab_find_partners_device("merge", p, ap))
        sts = R.step(p)
        ap = A.adapt_params(P, float(sts[0].dt))
        R.refused(1, lambda c: c.slab_adapt_device("merge", p, ap))
        R.refused(1, lambda c: c.slab_download_partner_decisions(infos[0]["participants"]))
        # closed by an upload_field of mass on ONE rank: every rank refuses the apply, together
        R.all(lambda c: c.classify(p))
        infos = R.all(lambda c: c.slab_find_partners_device("share", p, ap))
        R.grp[1].upload_field("mass", R.grp[1].download("mass"))
        assert status_of(R.grp[1].slab_download_partner_decisions, infos[0]["participants"])[0] == 1
        assert len(R.grp[0].slab_download_partner_decisions(infos[0]["participants"])[0]) == infos[0]["participants"]
        R.refused(1, lambda c: c.slab_adapt_device("share", p, ap), "no open solution")
        R.step(p)                                                                                  # every refusal left the ranks able to step
    finally:
        plain.close()
        close_all(loop)
        R.close()


def test_a_poisoned_rank(product_lib):
    """Ranks poisoned by a step that ran out of room answer SPH_ERR_POISONED."""
    scn = sc.dam_break_small(96, 48, 1 / 48)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    P = dam_break_params(max_iters=3, level_estimation_method="EmptyAngle", maximum_surface_distance=0.2, particle_radius_fine=0.004, particle_radius_base=0.02)
    p = P.to_ffi()
    ap = A.adapt_params(P, 1e-3)
    parts = D.partition(pos[:, 0], D.slab_cuts(pos[:, 0], 2))
    tg = D.ThreadedGroup(product_lib, pos, mass, vel, planes, 2, capacities=[len(q) + 8 for q in parts])
    try:
        with pytest.raises(ffi.SphError) as e:
            for _ in range(3):
                tg.step(p)
        assert e.value.status == 3
        for c in tg.contexts:
            assert status_of(c.slab_find_partners_device, "share", p, ap)[0] == 31
            assert status_of(c.slab_adapt_device, "share", p, ap)[0] == 31
            assert status_of(c.slab_download_partner_decisions, 0)[0] == 31
            assert status_of(c.slab_download_merged_partner_problem)[0] == 31
    finally:
        tg.close()


def test_one_rank_over_rccl_has_an_empty_relay(product_lib, monkeypatch):
    """A communicator of one rank, set up as tests/test_gpu_slabs.py::test_rccl_collectives_with_one_rank does: the table's all-reduce runs
    through RCCL, the relay has no round, the rank merges its own blob.  The decisions are those of sph_find_partners_device on a plain
    context that holds the same particles after the same steps."""
    P = default_params(**RADII)
    pos, mass, vel, planes = default_scene(P)
    p = P.to_ffi()
    plain = ffi.Context(product_lib, 70000, planes)
    monkeypatch.setenv("SPH_FORCE_SLAB_MODE", "1")
    raw = (C.c_uint8 * 128)()
    assert product_lib.comm_unique_id(raw) == 0
    c = ffi.Context(product_lib, 70000, planes)
    try:
        c.dist_configure(0, 1, -D.INF, D.INF)
        c.comm_init(bytes(raw), 0, 1)
        monkeypatch.delenv("SPH_FORCE_SLAB_MODE")
        plain.upload(mass, pos, vel)
        c.upload(mass, pos, vel)
        c.upload_field("particle_id", np.arange(len(mass), dtype=np.uint32))
        for _ in range(2):
            s0, s1 = plain.step(p), c.step(p)
        assert c.dist_get_stats()["transport"] == "rccl"
        ap = A.adapt_params(P, float(s1.dt))
        assert float(s0.dt) == float(s1.dt)
        print({f: same_bits(plain.download(f), D.gather_by_id([c], f, len(mass))) for f in ("mass", "position", "level_estimation", "h2")})
        for kind in ("share", "merge"):
            plain.classify(p)
            c.classify(p)
            want = plain.find_partners_device(kind, p, ap)
            got = c.slab_find_partners_device(kind, p, ap)
            assert bare(got) == want and got["participants"] > 0, (kind, got, want)
            K = want["participants"]
            ids0, mp0, mc0 = plain.download_partner_decisions(K)
            ids1, mp1, mc1 = c.slab_download_partner_decisions(K)
            order = c.download("particle_id")                        # the slab context's ids are the plain context's indices
            assert np.array_equal(np.sort(order), np.arange(len(mass)))
            assert np.array_equal(ids0, ids1) and np.array_equal(mp0, mp1) and np.array_equal(mc0, mc1), kind
            s = c.slab_relay_sizes()
            assert s["bytes_sent"] == s["bytes_received"] == 0 and len(s["bytes_of_rank"]) == 1 and s["bytes_of_rank"][0] > 0
            assert ffi.relay_plan(product_lib, 1, 0, 0, s["bytes_of_rank"], s["chunk_bytes"]) == []
            if kind == "share":
                plain.share_particles_device(p, ap)
                c.slab_adapt_device("share", p, ap)                  # (the merge below is searched behind the applied share on both)
        c.step(p)
    finally:
        plain.close()
        c.close()
