"""The compact partner problem on the device (include/sph_partner_problem.h): sph_download_partner_problem against
adaptivity.partner_problem_reference applied to the device's own full lists and fields, array for array; the compact apply calls against
sph_share_particles / sph_merge_particles on the expanded decisions (bit-identical states); the adaptive driver in export="compact"
mode against export="lists"; the refusals."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from adaptive_sph_amd import adaptivity as A, ffi, scene as sc
from adaptive_sph_amd.simulation import init_fluid_sim
from adaptive_sph_amd.workloads import default_params

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parent.parent
PATTERNS = REPO / "tests" / "golden" / "split-patterns.yaml"
RADII = dict(particle_radius_fine=0.012, particle_radius_base=0.05, maximum_surface_distance=0.3)   # test_share_and_merge_match_the_oracle
ALLOW = ["allow_share_with_optimal_particle", "allow_share_with_too_small_particle", "allow_merge_with_optimal_particle",
         "allow_merge_on_size_difference"]
DECISION_FIELDS = ("particle_size_class", "mass", "level_estimation", "position", "h2")
NAMES = ("ids",) + DECISION_FIELDS + ("offsets", "indices")
SCAN_TILE = 2048   # device_exclusive_scan_u32: items per block


def default_scene():
    scn = sc.SceneConfig.from_yaml(str(REPO / "tests" / "golden" / "default-scene.yaml"))
    pos, mass, vel = sc.init_particles(scn)
    return pos, mass, vel, sc.boundary_planes(scn.boundary)


def stepped(lib, P, steps=2, policy=None, cap=70000):
    pos, mass, vel, planes = default_scene()
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


def same_problem(got, ref, label):
    assert len(got) == len(ref) == len(NAMES)
    for name, a, b in zip(NAMES, got, ref):
        assert a is not None, (label, name)
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (label, name, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (label, name)


def test_problem_against_the_reference(product_lib):
    """FAST and EXACT policy, the step's lists and the extended lists of the advected positions (level_estimation_after_advection), the
    four allow_* flags off and on, both kinds; with and without persistent host buffers; as the first export of the step (the problem
    call builds the lists on the device itself) and after sph_download_neighbors."""
    participants = entries = 0
    for policy in ("fast", "exact"):
        for after in (False, True):
            P0 = default_params(level_estimation_after_advection=after, **RADII)
            g, p, dt = stepped(product_lib, P0, policy=policy)
            g.classify(p)
            ap0 = A.adapt_params(P0, dt)
            early = {k: g.download_partner_problem(k, p, ap0, want_ids=True) for k in ("share", "merge")}   # before any other export of this step
            off, idx = g.download_neighbors()
            f = [g.download(k) for k in DECISION_FIELDS]
            host = ffi.HostBuffers()
            for allow in (False, True):
                P = P0.replace(**{a: allow for a in ALLOW})
                ap = A.adapt_params(P, dt)
                for kind in ("share", "merge"):
                    label = (policy, after, allow, kind)
                    ref = A.partner_problem_reference(kind, *f, off, idx, P)
                    got = [g.download_partner_problem(kind, p, ap, want_ids=True), g.download_partner_problem(kind, p, ap, host, want_ids=True)]
                    if not allow:
                        got.append(early[kind])
                    for k, prob in enumerate(got):
                        same_problem(prob, ref, label + (k,))
                    assert g.download_partner_problem(kind, p, ap, host)[0] is None       # (ids only on request)
                    print(f"{label}: n={g.n} K={len(ref[0])} candidates={len(ref[7])}")
                    assert 0 < len(ref[0]) <= g.n, label
                    participants += len(ref[0])
                    entries += len(ref[7])
            g.step(p)   # the export poisoned nothing
            g.close()
    assert participants > 0 and entries > 0


def test_compact_apply_is_the_apply_on_the_expanded_arrays(product_lib):
    """Two contexts from the same upload.  A: the lists path (host decisions on the full lists, sph_share_particles, sph_classify,
    sph_merge_particles).  B: the compact path end to end, its merge problem taken after the share on the kept lists."""
    P = default_params(**RADII)
    a, p, dt = stepped(product_lib, P)
    b, _, _ = stepped(product_lib, P)
    ap = A.adapt_params(P, dt)
    a.classify(p)
    off, idx = a.download_neighbors()
    for kind in ("share", "merge"):
        a.classify(p)
        b.classify(p)
        f = [a.download(k) for k in DECISION_FIELDS]
        mp, mc = A._find_partners(kind, *f, off, idx, P, dt)
        ids, *fc, off_c, idx_c = b.download_partner_problem(kind, p, ap, want_ids=True)
        mp_c, mc_c = A._find_partners(kind, *fc, off_c, idx_c, P, dt)
        A.validate_partners(kind, fc[0], mp_c, mc_c, off_c, idx_c)
        emp, emc = A.expand_partner_decisions(b.n, ids, mp_c, mc_c)
        assert np.array_equal(mp, emp) and np.array_equal(mc, emc)
        print(f"{kind}: n={a.n} K={len(ids)} events={int(mc.sum())}")
        assert mc.sum() > 0 and mc_c.sum() == mc.sum()
        if kind == "share":
            a.share_particles(p, ap, mp, mc)
            b.share_particles_compact(p, ap, mp_c, mc_c)
        else:
            a.merge_particles(p, ap, mp, mc)
            b.merge_particles_compact(p, ap, mp_c, mc_c)
        assert a.n == b.n
        same_fields(all_fields(a), all_fields(b))
    assert a.n < len(mp)     # the merge deleted particles
    a.step(p)
    b.step(p)
    same_fields(all_fields(a), all_fields(b))


class _CaptureLists:
    def __init__(self, ctx):
        self.passes = []
        for name in ("share_particles", "merge_particles"):
            inner = getattr(ctx, name)

            def wrapped(p, ap, mp, mc, _inner=inner, _name=name):
                self.passes.append((_name, np.array(mp, copy=True), np.array(mc, copy=True)))
                return _inner(p, ap, mp, mc)
            setattr(ctx, name, wrapped)


class _CaptureCompact:
    """Asks every problem for its ids and keeps, per pass, the decisions expanded to the whole vector and (n, K)."""

    def __init__(self, ctx):
        self.passes, self.sizes, self.ids = [], [], None
        inner_problem = ctx.download_partner_problem

        def problem(kind, p, ap, host=None, want_ids=False):
            out = inner_problem(kind, p, ap, host, want_ids=True)
            self.ids = np.array(out[0], copy=True)
            return out
        ctx.download_partner_problem = problem
        for name in ("share_particles", "merge_particles"):
            inner = getattr(ctx, name + "_compact")

            def wrapped(p, ap, mp_c, mc_c, _inner=inner, _name=name):
                assert len(mp_c) == len(self.ids)
                self.passes.append((_name,) + A.expand_partner_decisions(ctx.n, self.ids, mp_c, mc_c))
                self.sizes.append((ctx.n, len(self.ids)))
                return _inner(p, ap, mp_c, mc_c)
            setattr(ctx, name + "_compact", wrapped)

            def forbidden(*a, _name=name):
                raise AssertionError(f"{_name} called in compact mode")
            setattr(ctx, name, forbidden)
        for name in ("download", "download_neighbors", "download_partner_candidates"):
            def forbidden(*a, _name=name):
                raise AssertionError(f"{_name} called in compact mode")
            setattr(ctx, name, forbidden)


def test_whole_driver_on_the_default_config(product_lib):
    """BASELINE configs[0] (default-config.yaml), 12 calls of single_step per mode from the same upload: the decisions of every pass
    (compact ones expanded through the problem's ids), the event counts, n and every downloadable field at the end are identical, and
    so is the state after one more plain step.  In compact mode the driver downloads no full field and no list."""
    scn = sc.SceneConfig.from_yaml(str(REPO / "tests" / "golden" / "default-scene.yaml"))
    P = default_params()
    sp = A.SplitPatterns.load_from_file(PATTERNS)
    sims = {m: init_fluid_sim(P, scn, lib=product_lib, split_patterns=sp, n_capacity=120000, adaptivity_export=m) for m in ("lists", "compact")}
    cl = _CaptureLists(sims["lists"].ctx)
    inner_download = {n: getattr(sims["compact"].ctx, n) for n in ("download", "download_neighbors")}
    cc = _CaptureCompact(sims["compact"].ctx)
    events = {m: {"shares": 0, "merges": 0, "splits": 0} for m in sims}
    participants = 0
    for s in range(12):
        for m, sim in sims.items():
            dt = sim.single_step_without_adaptivity(P)
            info = sim.single_step_adaptivity(P, dt)
            assert info["export"] == m
            for k in events[m]:
                events[m][k] += info[k]
            if m == "compact":
                assert len(cc.passes) > 0 and info["participants"] == sum(k for _, k in cc.sizes[-len(cc.passes):])   # (this step's passes)
                assert info["bytes_up"] == 6 * info["participants"]
                assert info["bytes_down"] == 25 * info["participants"] + 4 * len(cc.passes) + 4 * info["exported_indices"] + 16
                participants += info["participants"]
            else:
                assert info["participants"] == 0 and info["bytes_up"] > 0 and info["bytes_down"] > 4 * info["exported_indices"]
        assert len(cl.passes) == len(cc.passes) > 0
        for (n1, mp1, mc1), (n2, mp2, mc2) in zip(cl.passes, cc.passes):
            assert n1 == n2 and np.array_equal(mp1, mp2) and np.array_equal(mc1, mc2), (s, n1)
        cl.passes.clear()
        cc.passes.clear()
        assert events["lists"] == events["compact"], (s, events)
        assert sims["lists"].num_fluid_particles() == sims["compact"].num_fluid_particles()
    total_n = sum(n for n, _ in cc.sizes)
    print(f"configs[0]: events {events['lists']}, participants {participants} of {total_n} particle-passes, largest n {max(n for n, _ in cc.sizes)}")
    assert all(v > 0 for v in events["lists"].values()), events
    assert max(n for n, _ in cc.sizes) > SCAN_TILE        # the flag scan crossed a scan tile
    assert participants == sum(k for _, k in cc.sizes) and 0 < participants < total_n
    for n, f in inner_download.items():
        setattr(sims["compact"].ctx, n, f)
    same_fields(all_fields(sims["lists"].ctx), all_fields(sims["compact"].ctx))
    for sim in sims.values():
        sim.single_step_without_adaptivity(P)
    same_fields(all_fields(sims["lists"].ctx), all_fields(sims["compact"].ctx))
    for sim in sims.values():
        sim.close()


def test_the_download_writes_no_simulation_state(product_lib):
    P = default_params(**RADII)
    g, p, dt = stepped(product_lib, P, steps=1)
    twin, _, _ = stepped(product_lib, P, steps=1)
    ap = A.adapt_params(P, dt)
    for c in (g, twin):
        c.classify(p)
    before = all_fields(g)
    for kind in ("share", "merge"):
        assert len(g.download_partner_problem(kind, p, ap, want_ids=True)[0]) > 0
    same_fields(before, all_fields(g))
    g.step(p)
    twin.step(p)
    same_fields(all_fields(g), all_fields(twin))


def test_refusals(product_lib):
    from adaptive_sph_amd import distributed as D
    P = default_params(**RADII)
    pos, mass, vel, planes = default_scene()
    p = P.to_ffi()
    g = ffi.Context(product_lib, 70000, planes)
    g.upload(mass, pos, vel)
    ap = A.adapt_params(P, 1e-3)
    AV = A.MERGE_PARTNER_AVAILABLE

    def refused(status, f, *a):
        with pytest.raises(ffi.SphError) as e:
            f(*a)
        assert e.value.status == status, e.value

    def idle(k):
        return np.full(k, AV, np.uint32), np.zeros(k, np.uint16)

    def fresh_step():
        nonlocal ap
        ap = A.adapt_params(P, float(g.step(p).dt))
        g.classify(p)

    refused(1, g.download_partner_problem, "share", p, ap)               # before any step: no lists
    refused(1, g.share_particles_compact, p, ap, *idle(0))               # no open problem
    fresh_step()
    refused(1, g.merge_particles_compact, p, ap, *idle(0))               # lists, but still no open problem
    refused(1, g.download_partner_problem, 2, p, ap)                     # kind
    refused(1, g.download_partner_problem, "merge", None, ap)            # null params
    ids, *fc, off_c, idx_c = g.download_partner_problem("share", p, ap, want_ids=True)
    K = len(ids)
    assert K > 1 and len(idx_c) > 1
    before = all_fields(g)
    refused(1, g.merge_particles_compact, p, ap, *idle(K))               # the open problem is a share problem
    refused(1, g.share_particles_compact, p, ap, *idle(K + 1))           # k != K
    refused(1, g.share_particles_compact, p, ap, *idle(K - 1))
    bad = idle(K)
    bad[0][K - 1] = K                                                    # a compact id >= K
    refused(1, g.share_particles_compact, p, ap, *bad)
    same_fields(before, all_fields(g))                                   # ... and nothing was modified
    mp_c, mc_c = A._find_partners("share", *fc, off_c, idx_c, P, ap.dt)
    assert mc_c.sum() > 0
    g.share_particles_compact(p, ap, mp_c, mc_c)                         # the refusals left the problem open
    refused(1, g.share_particles_compact, p, ap, mp_c, mc_c)             # consumed: apply twice on one problem
    g.step(p)
    g.classify(p)
    # a problem made before sph_step / sph_upload and applied after it
    K = len(g.download_partner_problem("merge", p, ap, want_ids=True)[0])
    fresh_step()
    refused(1, g.merge_particles_compact, p, ap, *idle(K))
    K = len(g.download_partner_problem("merge", p, ap, want_ids=True)[0])
    g.upload(mass, pos, vel)
    refused(1, g.merge_particles_compact, p, ap, *idle(K))
    fresh_step()
    # capacities one too small: status 1 with both counts set, and no problem left open
    ids, *fc, off_c, idx_c = g.download_partner_problem("merge", p, ap, want_ids=True)
    K, T = len(ids), len(idx_c)
    assert K > 1 and T > 1
    k, t = C.c_uint64(0), C.c_uint64(0)
    buf = {n: np.empty(K * ffi.FIELDS[n][2], ffi.FIELDS[n][1]) for n in DECISION_FIELDS}
    o_ids, o_off, o_idx = np.empty(K, np.uint32), np.empty(K + 1, np.uint32), np.empty(T, np.uint32)

    def raw(pcap, icap):
        k.value = t.value = 0
        return product_lib.download_partner_problem(g.handle, 1, C.byref(p), C.byref(ap), o_ids.ctypes.data, *[buf[n].ctypes.data for n in DECISION_FIELDS],
                                                    o_off.ctypes.data, pcap, o_idx.ctypes.data, icap, C.byref(k), C.byref(t))

    assert raw(K - 1, T) == 1 and (int(k.value), int(t.value)) == (K, T)
    refused(1, g.merge_particles_compact, p, ap, *idle(K))
    assert raw(K, T - 1) == 1 and (int(k.value), int(t.value)) == (K, T)
    rc = product_lib.download_partner_problem(g.handle, 1, C.byref(p), C.byref(ap), None, None, None, None, None, None, None, 0, None, 0, C.byref(k), C.byref(t))
    assert rc == 0 and (int(k.value), int(t.value)) == (K, T)            # the sizing call
    assert raw(K, T) == 0 and np.array_equal(o_ids, ids) and np.array_equal(o_off, off_c) and np.array_equal(o_idx, idx_c)
    g.merge_particles_compact(p, ap, *idle(K))                           # (nobody merges: the vector stays as it is)
    assert g.n == len(mass)
    refused(1, g.download_partner_problem, "merge", p, ap)               # after a merge apply the lists are gone
    g.step(p)
    # a slab context (member of a loopback group): all three calls are unsupported, and the group steps afterwards
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 2)
    ffi.group_step(grp, p)
    refused(30, grp[0].download_partner_problem, "share", p, ap)
    refused(30, grp[0].share_particles_compact, p, ap, *idle(0))
    refused(30, grp[0].merge_particles_compact, p, ap, *idle(0))
    ffi.group_step(grp, p)
