"""Probe sets on slab contexts (include/sph_slab_probe.h) against the numpy restatement of the probe sums (tests/probe_reference.py) and of
the compact layers (tests/slab_probe_reference.py), bit for bit: the ranks' layers word for word, the composed words and resolved
values through the group call and through the per-rank calls, lattice centres against sample_group, the ranks' agreement on the
exponents and on the refusal, that no word depends on the bins, tracers on every replica, that probing changes no state, and the
refusals.

The expectation is always numpy fed with the GROUP's own fields assembled by global id -- never a plain context stepped beside it.
Every comparison is np.array_equal on int64 words or on float32 bit patterns."""
import ctypes as C

import numpy as np
import pytest

from adaptive_sph_amd import distributed as D, ffi, probes, sampling, scene as sc
from adaptive_sph_amd.workloads import default_params
from tests import probe_reference as pr, sample_reference as sr, slab_probe_reference as spr, slab_sample_reference as ssr
from tests.test_gpu_slab_render import FIELDS, Group, _scene_a, _scene_b, close_all

pytestmark = pytest.mark.gpu

CH = ["density", "pressure", "velocity_x", "velocity_y", "level_estimation"]
VEL = ["velocity_x", "velocity_y"]
FIXTURES = ["A2", "A3", "B2", "B3"]


@pytest.fixture(scope="module")
def groups(product_lib):
    """which -> the loopback group of tests/test_gpu_slab_render.py (scene A: the 40 x 32 dam break, 4 steps; scene B: the 2:1 media scene,
    3 steps; k = 2 or 3 slabs), built on first use, gathered once and left unchanged."""
    made = {}

    def get(which):
        if which not in made:
            g = (_scene_a if which[0] == "A" else _scene_b)(product_lib, int(which[1]))
            assert all(len(i) > 0 for i in g.ids)
            g.own = [np.sort(i).astype(np.int64) for i in g.ids]
            made[which] = g
        return made[which]

    yield get
    for g in made.values():
        g.close()


class Replicas:
    """One ProbeSet per member of a group, the same points in the same order."""

    def __init__(self, g, pts, cells=None):
        self.pts = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 2))
        self.sets = [probes.ProbeSet(c, self.pts, 0.0 if cells is None else cells[r]) for r, c in enumerate(g.ctxs)]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for s in self.sets:
            s.close()


def _particles(g, channels=CH, volume="density"):
    return pr.Particles(g.f, channels, g.P.rest_density, g.P.maximum_surface_distance, volume)


def _twin(g, pts, channels=CH, volume="density", exps=None):
    """-> {"exps", "whole": (raw, foot, touched), "rank": [(indices, words, foot)]} for the whole vector and every rank's owned particles"""
    tw = _particles(g, channels, volume)
    used = pr.exponents(tw) if exps is None else list(exps)
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    return {"exps": used, "whole": pr.raw_at_points(tw, used, pts[:, 0], pts[:, 1]),
            "rank": [spr.layer(tw, own, used, pts[:, 0], pts[:, 1]) for own in g.own]}


def _pp(channels, exps=None, **kw):
    return probes.probe_params(sampling.expand_channels(channels), exponents=exps, **kw)


def _layers(g, rep, pp):
    """Every member's layer call and download -> [(indices, words, info)]"""
    out = []
    for c, s in zip(g.ctxs, rep.sets):
        info = c.slab_probe_layer(g.p, s.handle, pp)
        n = int(info.n_entries)
        idx, words = c.slab_probe_layer_download(s.handle) if n else (None, None)   # (no entries: no download needed)
        out.append((idx, words, info))
    return out


def _rank_path(g, rep, channels=CH, exps=None, on=0, order=None, **kw):
    """The per-rank calls on every member, the fold, the compose on member `on` -> (raw, values, folded pp, layers, info)"""
    pp = _pp(channels, exps, **kw)
    words = [c.slab_probe_range(g.p, pp) for c in g.ctxs]
    pp = ffi.probe_fold_words(g.ctxs[0].lib, words, pp)
    layers = _layers(g, rep, pp)
    order = list(range(len(layers))) if order is None else order
    values, raw, info = g.ctxs[on].probe_compose(rep.sets[on].handle, pp, len(rep.pts), [None if layers[i][0] is None else layers[i][:2] for i in order], raw=True)
    return raw, values, pp, layers, info


def _group_path(g, rep, channels=CH, **kw):
    v = probes.sample_group(g.ctxs, rep.sets, g.P, channels, raw=True, **kw)
    return np.stack([v.raw[k] for k in ["weight"] + v.names]), np.stack([v.weight] + [v.values[k] for k in v.names]), v


def _diff(a, b):
    return [int(np.count_nonzero(a[k] != b[k])) for k in range(len(a))]


def _resolve(raw, exps, **kw):
    return sampling.resolve(raw[:, None, :], exps, **kw)[:, 0]


def _random_over(g, n, seed, margin=0.15):
    lo, hi = g.f["position"].min(axis=0) - margin, g.f["position"].max(axis=0) + margin
    return np.random.default_rng(seed).uniform(lo, hi, (n, 2)).astype(np.float32)


def _in_fluid(g, n, seed, among=None):
    rng = np.random.default_rng(seed)
    j = rng.integers(0, g.n, n) if among is None else among[rng.integers(0, len(among), n)]
    return (g.f["position"][j] + rng.uniform(-1, 1, (n, 2)) * g.f["h2"][j, None]).astype(np.float32)


def _check_layers(g, pts, channels=CH, volume="density", label=""):
    tw = _twin(g, pts, channels, volume)
    pp = _pp(channels, tw["exps"], volume=volume)
    with Replicas(g, pts) as rep:
        got = _layers(g, rep, pp)
    for r, ((idx, words, info), (w_idx, w_words, foot)) in enumerate(zip(got, tw["rank"])):
        assert int(info.n_entries) == len(w_idx), (label, r, int(info.n_entries), len(w_idx))
        if len(w_idx):
            assert idx.dtype == np.uint32 and np.array_equal(idx, w_idx), (label, r)
            assert words.shape == w_words.shape and np.array_equal(words, w_words), (label, r, _diff(words, w_words))
        assert (int(info.n_touching), int(info.n_pairs)) == (int((foot > 0).sum()), int(foot.sum())), (label, r)
        assert list(info.exponents)[:len(channels)] == tw["exps"]
    whole, foot, touched = tw["whole"]
    assert sum(int(i.n_pairs) for _, _, i in got) == int(foot.sum()) and sum(int(i.n_touching) for _, _, i in got) == int((foot > 0).sum())
    composed, seen = spr.compose(len(channels) + 1, len(np.asarray(pts).reshape(-1, 2)), [t[:2] for t in tw["rank"]])
    assert np.array_equal(composed, whole) and np.array_equal(seen, touched)
    return tw, got


# ---- 1. layers word for word -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("volume", ["density", "rest"])
@pytest.mark.parametrize("which", FIXTURES)
def test_layers_word_for_word_random_points(groups, which, volume):
    g = groups(which)
    tw, got = _check_layers(g, _random_over(g, 300, 5), volume=volume, label=(which, volume))
    assert all(0 < int(i.n_entries) < 300 for _, _, i in got) and (~tw["whole"][2]).any()


def test_layers_all_in_one_ranks_interior(groups):
    g = groups("A3")
    x = g.f["position"][:, 0]
    reach = 2.2 * float(g.f["h2"].max())
    inner = g.own[0][x[g.own[0]] < float(x[g.own[1]].min()) - 2 * reach]      # rank 0's particles further than two supports from rank 1's
    assert len(inner) > 20
    pts = (g.f["position"][inner[:80]] + np.float32(0.003)).astype(np.float32)
    tw, got = _check_layers(g, pts, label="interior")
    assert int(got[0][2].n_entries) == len(pts) and all(int(i.n_entries) == 0 and idx is None for idx, _, i in got[1:])


@pytest.mark.parametrize("which", ["A2", "B3"])
def test_layers_on_and_beside_the_cuts(groups, which):
    g = groups(which)
    x = g.f["position"][:, 0]
    h = float(g.f["h2"].max())
    ys = np.linspace(float(g.f["position"][:, 1].min()), float(g.f["position"][:, 1].max()), 12)
    pts = []
    for r in range(len(g.own) - 1):
        cut = 0.5 * (float(x[g.own[r]].max()) + float(x[g.own[r + 1]].min()))
        for dx in (-2 * h, -h, -0.5 * h, 0.0, 0.5 * h, h, 2 * h):
            pts += [(cut + dx, y) for y in ys]
    tw, got = _check_layers(g, np.array(pts, np.float32), label=("cuts", which))
    for r in range(len(g.own) - 1):                                           # two ranks contribute to the same point
        both = np.intersect1d(tw["rank"][r][0], tw["rank"][r + 1][0])
        assert len(both) > 0 and len(np.intersect1d(got[r][0], got[r + 1][0])) == len(both), r


def test_layers_far_outside_copies_and_clusters(groups):
    g = groups("B2")
    rng = np.random.default_rng(9)
    inside = _in_fluid(g, 40, 10)
    far = np.stack([rng.uniform(50.0, 60.0, 30), rng.uniform(-80.0, -70.0, 30)], axis=1).astype(np.float32)   # untouched points
    cluster = (inside[3] + rng.uniform(-1e-4, 1e-4, (50, 2))).astype(np.float32)
    pts = np.concatenate([inside, far, np.repeat(inside[:5], 7, axis=0), cluster, inside[::-1]])             # exact copies, a cluster
    tw, got = _check_layers(g, pts, label="copies")
    touched = tw["whole"][2]
    assert not touched[40:70].any() and touched[:40].all()
    _check_layers(g, far, label="far")                                                                       # no rank touches anything


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_layers_small_sets(groups, n):
    g = groups("A2")
    x = g.f["position"][:, 0]
    cut = 0.5 * (float(x[g.own[0]].max()) + float(x[g.own[1]].min()))
    near = np.flatnonzero(np.abs(x - cut) < float(g.f["h2"].max()))
    pts = _in_fluid(g, 65, 3, among=near)[:n]
    tw, got = _check_layers(g, pts, label=n)
    with Replicas(g, pts) as rep:
        raw, values, v = _group_path(g, rep)
        assert raw.shape == (len(CH) + 1, n) and np.array_equal(raw, tw["whole"][0]) and np.array_equal(_rank_path(g, rep)[0], tw["whole"][0])
        assert (v.n_touching, v.n_pairs, v.n_touched_points) == (int((tw["whole"][1] > 0).sum()), int(tw["whole"][1].sum()), int(tw["whole"][2].sum()))
        assert list(v.exponents.values()) == tw["exps"]
    assert n == 0 or raw[0].any()


def test_layers_across_the_scan_tiles(groups):
    """4 097 points: the pack's scan crosses its tile of 2 048 twice."""
    g = groups("A2")
    pts = np.concatenate([_random_over(g, 1097, 22, margin=0.5), _in_fluid(g, 3000, 21)])
    assert len(pts) == 4097
    tw, got = _check_layers(g, pts, ["density", "velocity_x"], label="4097")
    assert (~tw["whole"][2]).any()
    for idx, _, info in got:                                                 # every rank has entries in the first two tiles ...
        assert int(info.n_entries) > 1000 and (idx < 2048).any() and ((idx >= 2048) & (idx < 4096)).any() and idx[1000] > 1000
    assert any(idx[-1] == 4096 for idx, _, _ in got)                         # ... and the point alone in the third is an entry


# ---- 2. composed raw words and resolved values ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("volume", ["density", "rest"])
@pytest.mark.parametrize("which", FIXTURES)
def test_composed_words_and_values(groups, product_lib, which, volume):
    g = groups(which)
    k = len(g.ctxs)
    pts = np.concatenate([_random_over(g, 200, 6), _in_fluid(g, 100, 7)])
    tw = _twin(g, pts, CH, volume)
    want, foot, touched = tw["whole"]
    counts = (int((foot > 0).sum()), int(foot.sum()), int(touched.sum()))
    with Replicas(g, pts) as rep:
        for normalize in (False, True):
            kw = dict(volume=volume, normalize=normalize, min_weight=0.5, fill=float("nan"))
            res = _resolve(want, tw["exps"], normalize=normalize, min_weight=0.5, fill=float("nan"))
            nan = np.isnan(res)
            assert nan.any() == normalize and not nan[0].any()
            raw, values, v = _group_path(g, rep, **kw)
            assert np.array_equal(raw, want), (which, volume, "group", _diff(raw, want))
            assert list(v.exponents.values()) == tw["exps"] and (v.n_touching, v.n_pairs, v.n_touched_points) == counts
            raw2, values2, pp, layers, info = _rank_path(g, rep, **kw)
            assert np.array_equal(raw2, want), (which, volume, "per rank", _diff(raw2, want))
            assert [pp.channels[c].exponent for c in range(len(CH))] == tw["exps"]
            assert int(info.n_touched_points) == counts[2] and (int(info.n_touching), int(info.n_pairs)) == (0, 0)
            for got in (values, values2):
                assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], res.view(np.uint32)[~nan])
        # layers handed in reversed order, composed on the last member; composed on a PLAIN context that owns a set with the same points
        raw3 = _rank_path(g, rep, volume=volume, on=k - 1, order=list(range(k))[::-1])[0]
        assert np.array_equal(raw3, want)
        plain = ffi.Context(product_lib, 16, g.planes)
        try:
            with probes.ProbeSet(plain, pts) as ps:
                _, raw4, info = plain.probe_compose(ps.handle, pp, len(pts), [l[:2] for l in layers], raw=True)
                assert np.array_equal(raw4, want) and int(info.n_touched_points) == counts[2]
                values0, raw0, info = plain.probe_compose(ps.handle, pp, len(pts), [], raw=True)            # no layers: all-zero planes
                assert not raw0.any() and not values0[0].any() and int(info.n_touched_points) == 0
        finally:
            plain.close()


# ---- 3. lattice centres ----------------------------------------------------------------------------------------------------------
def test_lattice_centres_get_the_group_samples_words(groups):
    g = groups("A3")
    lo = g.f["position"].min(axis=0) - 0.1
    grid = sampling.GridSpec(23, 17, (float(lo[0]), float(lo[1])), 0.06)
    X, Y = sr.centers(grid.nx, grid.ny, grid.origin, grid.spacing)
    pts = np.stack([np.tile(X, grid.ny), np.repeat(Y, grid.nx)], axis=1)
    lattice = sampling.sample_group(g.ctxs, g.P, grid, CH, raw=True)
    lat = np.stack([lattice.raw[k] for k in ["weight"] + CH])
    with Replicas(g, pts) as rep:
        raw, values, v = _group_path(g, rep)
        raw2 = _rank_path(g, rep)[0]
    assert lat[0].any() and np.array_equal(raw.reshape(lat.shape), lat) and np.array_equal(raw2.reshape(lat.shape), lat)
    assert list(v.exponents.values()) == list(lattice.exponents.values()) and (v.n_touching, v.n_pairs) == (lattice.n_touching, lattice.n_pairs)
    assert np.array_equal(values.reshape(lat.shape).view(np.uint32), np.stack([lattice.planes[k] for k in ["weight"] + CH]).view(np.uint32))


# ---- 4. agreement ----------------------------------------------------------------------------------------------------------------
def test_ranks_agree_on_the_exponents(groups):
    differ = []
    for which in FIXTURES:
        g = groups(which)
        tw = _particles(g)
        whole = pr.exponents(tw)
        pp = _pp(CH)
        words = [c.slab_probe_range(g.p, pp) for c in g.ctxs]
        own = []
        for r, w in enumerate(words):
            assert w.as_tuple() == ssr.words(tw.subset(g.own[r]), g.own[r]) and w.first_bad == ffi.SAMPLE_NO_OFFENDER, (which, r)
            own.append(ssr.fold_words([w.as_tuple()], CH, [None] * len(CH))[1])
        folded = ffi.probe_fold_words(g.ctxs[0].lib, words, pp)
        assert [folded.channels[c].exponent for c in range(len(CH))] == whole
        with Replicas(g, _in_fluid(g, 10, 1)) as rep:
            assert list(probes.sample_group(g.ctxs, rep.sets, g.P, CH).exponents.values()) == whole
        differ += [(which, CH[c]) for c in range(len(CH)) if len({e[c] for e in own}) > 1]
    assert differ, "every rank's own maxima give the whole vector's exponents on every fixture: the test shows nothing"


@pytest.mark.parametrize("which", ["A2", "A3"])   # (scene B's columns stand still in x: no velocity_x to refuse)
def test_one_refusal_on_every_path(groups, which):
    g = groups(which)
    tw = _particles(g)
    vx = np.abs(g.f["velocity"][:, 0])
    tops = sorted(float(vx[own].max()) for own in g.own)
    e = sr.exponent_of(tops[-2]) - 1                     # 2^e <= the second largest of the ranks' maxima: two ranks reach it
    assert sum(bool((vx[own] >= 2.0 ** e).any()) for own in g.own) >= 2
    exps = [None, None, e, None, None]
    idx, why = pr.first_offender(tw, exps)
    assert why == sr.BAD_CHANNEL + 2
    kind, sentence = ssr.fold_words([ssr.words(tw.subset(own), own, exps) for own in g.own], CH, exps)
    assert kind == "refused" and f"(particle i={idx})" in sentence
    pts = _in_fluid(g, 50, 2)
    want = _twin(g, pts)["whole"][0]
    with Replicas(g, pts) as rep:
        with pytest.raises(ffi.SphError) as err:
            probes.sample_group(g.ctxs, rep.sets, g.P, CH, exponents=exps)
        assert err.value.status == 1 and sentence in str(err.value), (err.value, sentence)
        pp = _pp(CH, exps)
        words = [c.slab_probe_range(g.p, pp) for c in g.ctxs]
        assert sum(w.first_bad != ffi.SAMPLE_NO_OFFENDER for w in words) >= 2
        for order in (words, words[::-1]):
            with pytest.raises(ffi.SphError) as err:
                ffi.probe_fold_words(g.ctxs[0].lib, order, pp)
            assert err.value.status == 1 and str(err.value).endswith(sentence), (err.value, sentence)
        # the tracer step refuses the same particle through its own two channels; no point moved
        with pytest.raises(ffi.SphError, match=rf"channel 0 \(velocity\).*\(particle i={idx}\)") as err:
            probes.advect_group(g.ctxs, rep.sets, g.P, 0.001, exponents=[e, None])
        assert err.value.status == 1 and all(np.array_equal(s.points(), pts) for s in rep.sets)
        assert np.array_equal(_group_path(g, rep)[0], want)   # nothing changed: the next sample is the twin's


# ---- 5. no word depends on the bins ----------------------------------------------------------------------------------------------
def test_no_word_depends_on_the_bins(groups):
    g = groups("B3")
    pts = np.concatenate([_random_over(g, 150, 12), _in_fluid(g, 150, 13)])
    want = _twin(g, pts)["whole"][0]
    h = g.f["h2"]
    for cells in ([0.0, 0.5 * float(h.min()), 10.0 * float(h.max())], [100.0, 0.0, 1e-6]):    # one cell; capped at 2^22 cells
        with Replicas(g, pts, cells) as rep:
            assert len({s.bins() for s in rep.sets}) == 3
            assert np.array_equal(_group_path(g, rep)[0], want) and np.array_equal(_rank_path(g, rep)[0], want), cells


# ---- 6. tracers ------------------------------------------------------------------------------------------------------------------
def test_tracers_on_every_replica(product_lib):
    P = default_params(merging=False, sharing=False, splitting=False, constrain_neighborhood_count=True, max_dt=0.004, maximum_surface_distance=0.2)
    scn = sc.dam_break_small(40, 32, 1.0 / 40)
    pos0 = sc.init_particles(scn)[0]
    start = np.ascontiguousarray(pos0[::3], np.float32)
    # the cut runs 0.002 to the right of a column of tracers, a fifth of the column's width behind the dam's face: the collapsing face
    # carries them across it
    x_face = float(pos0[:, 0].max())
    x_col = float(start[np.argmin(np.abs(start[:, 0] - (x_face - 0.2))), 0])
    cut = x_col + 0.002
    g = Group(product_lib, scn, P, 2, 1, [[-D.INF, cut, D.INF]])
    try:
        assert abs(g.ctxs[0].dist_get_cuts()[1] - cut) < 1e-6 and all(len(i) > 100 for i in g.ids)
        with Replicas(g, start) as grp, Replicas(g, start) as per_rank:
            now = start
            side0 = now[:, 0] < cut
            crossed = np.zeros(len(now), bool)
            for step in range(80):
                if step >= 20 and crossed.any():                             # 20 steps at least; longer until a tracer has crossed
                    break
                dt = float(ffi.group_step(g.ctxs, g.p)[0].dt)
                g.gather()
                g.own = [np.sort(i).astype(np.int64) for i in g.ids]
                tw = _particles(g, VEL, "rest")
                exps = pr.exponents(tw)
                ranks = [spr.layer(tw, own, exps, now[:, 0], now[:, 1]) for own in g.own]
                raw, _ = spr.compose(3, len(now), [t[:2] for t in ranks])
                X, Y, moved = pr.advect(raw, exps, now[:, 0], now[:, 1], dt, 0.5)
                want = np.stack([X, Y], axis=1)
                info = probes.advect_group(g.ctxs, grp.sets, P, dt)
                assert (int(info.n_moved), int(info.n_stalled)) == (int(moved.sum()), int((~moved).sum())) and info.n_moved + info.n_stalled == len(now)
                assert [info.exponents[0], info.exponents[1]] == exps and int(info.n_pairs) == sum(int(t[2].sum()) for t in ranks)
                for r, s in enumerate(grp.sets):
                    got = s.points()
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("group", step, r, int(np.count_nonzero(got != want)))
                # the per-rank calls driven in one process: the layers of all members handed to compose_advect on each
                ap = probes._advect_params(dt)
                pp = ffi.probe_fold_words(product_lib, [c.slab_probe_range(g.p, probes._velocity_params(ap)) for c in g.ctxs], probes._velocity_params(ap))
                assert [pp.channels[0].exponent, pp.channels[1].exponent] == exps
                ap.exponent_x, ap.exponent_y = exps
                layers = _layers(g, per_rank, pp)
                for r, (c, s) in enumerate(zip(g.ctxs, per_rank.sets)):
                    one = c.probe_compose_advect(s.handle, ap, [None if l[0] is None else l[:2] for l in (layers if r == 0 else layers[::-1])])
                    assert (int(one.n_moved), int(one.n_stalled)) == (int(moved.sum()), int((~moved).sum()))
                    got = s.points()
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), ("per rank", step, r, int(np.count_nonzero(got != want)))
                now = want
                crossed |= (now[:, 0] < cut) != side0
            print("tracers: steps", step, "crossed", int(crossed.sum()))
            assert crossed.any(), "no tracer crossed the cut: lengthen the run"
    finally:
        g.close()


# ---- 7. read-only ----------------------------------------------------------------------------------------------------------------
def test_probing_changes_no_state(product_lib):
    """Two identical 2-slab groups; one samples and advects between steps through the group calls and the per-rank calls: every
    downloadable field, the ids and the exported lists stay equal byte for byte."""
    P = default_params(merging=False, sharing=False, splitting=False, max_dt=0.004, maximum_surface_distance=0.2)
    scn = sc.dam_break_small(32, 32, 1.0 / 32)
    a = Group(product_lib, scn, P, 2, 2)
    b = Group(product_lib, scn, P, 2, 2)
    try:
        a.own = [np.sort(i).astype(np.int64) for i in a.ids]
        with Replicas(a, _in_fluid(a, 200, 4)) as rep:
            for _ in range(2):
                assert _group_path(a, rep, normalize=True)[0].any() and _rank_path(a, rep, volume="rest")[0].any()
                assert probes.advect_group(a.ctxs, rep.sets, P, 0.002).n_moved > 0
                ffi.group_step(a.ctxs, a.p)
                ffi.group_step(b.ctxs, b.p)
            for x, y in zip(a.ctxs, b.ctxs):
                for f in FIELDS + ["particle_id", "cell_index", "h2_next", "level_old", "lambda_sum"]:
                    assert x.download(f).tobytes() == y.download(f).tobytes(), f
                (oa, ia), (ob, ib) = x.download_neighbors(), y.download_neighbors()
                assert np.array_equal(oa, ob) and np.array_equal(ia, ib)
            # a layer is a read-out: it outlives the steps and the advect
            n = int(a.ctxs[0].slab_probe_layer(a.p, rep.sets[0].handle, _pp(["density"], [11])).n_entries)
            ffi.group_step(a.ctxs, a.p)
            assert n > 0 and a.ctxs[0].slab_probe_layer_download(rep.sets[0].handle)[1][0].all()
    finally:
        a.close()
        b.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(product_lib):
    P = default_params(merging=False, sharing=False, splitting=False, max_dt=0.004)
    scn = sc.dam_break_small(32, 32, 1.0 / 32)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    p = P.to_ffi()
    lib = product_lib
    plain = ffi.Context(lib, len(mass) + 64, planes)
    grp = D.make_loopback_group(lib, pos, mass, vel, planes, 2)
    pts = (pos[::5] + np.float32(0.01)).astype(np.float32)
    n = len(pts)
    ch = ["density", "velocity"]
    names = sampling.expand_channels(ch)

    def refused(status, match, fn, *a, **kw):
        with pytest.raises(ffi.SphError, match=match) as e:
            fn(*a, **kw)
        assert e.value.status == status, e.value

    try:
        plain.upload(mass, pos, vel)
        plain_set = probes.ProbeSet(plain, pts)
        sets = [probes.ProbeSet(c, pts) for c in grp]
        handles = [s.handle for s in sets]
        pp1, auto = _pp(["density"], [11]), _pp(["density"])
        ap = probes._advect_params(0.001, exponents=[3, 3])
        ap_auto = probes._advect_params(0.001)
        # before the first step h is 0: the data precondition, through the group calls and the fold
        refused(1, r"particle i=0; before the first step", probes.sample_group, grp, sets, P, ch)
        refused(1, r"particle i=0; before the first step", probes.advect_group, grp, sets, P, 0.001)
        refused(1, r"particle i=0; before the first step", ffi.probe_fold_words, lib, [c.slab_probe_range(p, auto) for c in grp], auto)
        refused(1, "no layer", grp[0].slab_probe_layer_download, handles[0])                 # a download before any layer
        ffi.group_step(grp, p)
        own = [np.sort(c.download("particle_id")).astype(np.int64) for c in grp]
        f = {k: D.gather_by_id(grp, k, len(mass)) for k in FIELDS}
        tw = pr.Particles(f, names, P.rest_density, P.maximum_surface_distance)
        exps = pr.exponents(tw)
        want = pr.raw_at_points(tw, exps, pts[:, 0], pts[:, 1])[0]
        ppx = _pp(ch, exps)
        good = []
        for c, s in zip(grp, sets):
            info = c.slab_probe_layer(p, s.handle, ppx)
            good.append(c.slab_probe_layer_download(s.handle))
            assert good[-1][1].shape == (len(names) + 1, int(info.n_entries))
        assert all(len(l[0]) > 3 for l in good)

        def still_right():
            v = probes.sample_group(grp, sets, P, ch, raw=True)
            assert np.array_equal(np.stack([v.raw[k] for k in ["weight"] + names]), want)
            assert np.array_equal(grp[1].probe_compose(handles[1], ppx, n, good, raw=True)[1], want)
            assert all(np.array_equal(s.points(), pts) for s in sets + [plain_set])                 # no refused call moved a point

        def refused_then_right(status, match, fn, *a, **kw):
            refused(status, match, fn, *a, **kw)
            still_right()

        still_right()
        # SPH_ERR_UNSUPPORTED: range, layer, download on a plain context; a plain group member; sample / advect on a slab context
        hint = "sph_probe_sample samples a plain context"
        refused_then_right(30, hint, plain.slab_probe_range, p, pp1)
        refused_then_right(30, hint, plain.slab_probe_layer, p, plain_set.handle, pp1)
        refused_then_right(30, hint, plain.slab_probe_layer_download, plain_set.handle)
        refused_then_right(30, hint, ffi.group_probe_sample, [grp[0], plain], p, [handles[0], plain_set.handle], pp1, n)
        refused_then_right(30, hint, ffi.group_probe_sample, [plain, grp[0]], p, [plain_set.handle, handles[0]], pp1, n)
        refused_then_right(30, hint, ffi.group_probe_advect, [grp[0], plain], p, [handles[0], plain_set.handle], ap)
        refused_then_right(30, r"raw sums of disjoint particle sets add exactly.*sample_group / ProbeSet\.sample_rank", sets[0].sample, P, ["density"])
        refused_then_right(30, r"raw sums of disjoint particle sets add exactly.*advect_group / ProbeSet\.advect_rank", sets[0].advect, P, 0.001)
        with pytest.raises(ffi.SphError) as e:                                                     # the status name stands once, in front
            sets[0].sample(P, ["density"])
        assert str(e.value).startswith("SPH_ERR_UNSUPPORTED: probe: slab contexts") and str(e.value).count("SPH_ERR_UNSUPPORTED") == 1, str(e.value)
        # automatic exponents where the fold comes first
        refused_then_right(1, "the fold comes first", grp[0].slab_probe_layer, p, handles[0], auto)
        kept = lib.slab_probe_layer_download                                                       # (a refused layer call leaves the kept layer)
        idx0, wds0 = np.empty_like(good[0][0]), np.empty_like(good[0][1])
        assert kept(grp[0].handle, handles[0], idx0.ctypes.data, wds0.ctypes.data, len(idx0)) == 0
        assert np.array_equal(idx0, good[0][0]) and np.array_equal(wds0, good[0][1])
        refused_then_right(1, "the fold comes first", plain.probe_compose, plain_set.handle, auto, n, [])
        refused_then_right(1, "the fold comes first", grp[0].probe_compose_advect, handles[0], ap_auto, [])
        # null arguments
        refused_then_right(1, "null", grp[0].slab_probe_range, None, pp1)
        refused_then_right(1, "null", grp[0].slab_probe_range, p, None)
        refused_then_right(1, "null", grp[0].slab_probe_layer, None, handles[0], pp1)
        refused_then_right(1, "null", grp[0].slab_probe_layer, p, handles[0], None)
        refused_then_right(1, "null", grp[0].probe_compose, handles[0], None, n, [])
        refused_then_right(1, "null", grp[0].probe_compose_advect, handles[0], None, [])
        refused_then_right(1, "null", ffi.group_probe_sample, grp, None, handles, pp1, n)
        refused_then_right(1, "null", ffi.group_probe_sample, grp, p, handles, None, n)
        refused_then_right(1, "null", ffi.group_probe_advect, grp, None, handles, ap)
        refused_then_right(1, "null", ffi.group_probe_advect, grp, p, handles, None)
        assert lib.slab_probe_range(grp[0].handle, C.byref(p), C.byref(pp1), None) == 1
        # every channel, volume and exponent refusal of sph_probe_sample, on every call that takes them
        q7 = _pp(["density"] * 6, [1] * 6)
        q7.n_channels = 7
        qf = _pp(["density", "pressure"], [11, 13])
        qf.channels[1].field = ffi.FIELDS["mass"][0]
        qc = _pp(["density", "pressure"], [11, 13])
        qc.channels[1].component = 1
        qv = _pp(["density"], [11])
        qv.volume = 2
        for q, word in ((q7, "7 channels"), (qf, "cannot be sampled"), (qc, "pressure has no component 1"), (_pp(["density"], [65]), "exponent 65"), (qv, "volume mode")):
            refused_then_right(1, word, ffi.group_probe_sample, grp, p, handles, q, n)
            refused(1, word, grp[1].slab_probe_range, p, q)
            refused(1, word, grp[1].slab_probe_layer, p, handles[1], q)
            refused(1, word, plain.probe_compose, plain_set.handle, q, n, [])
        bad_ap = probes._advect_params(0.001, exponents=[3, 3])
        bad_ap.volume = 2
        refused_then_right(1, "volume mode", ffi.group_probe_advect, grp, p, handles, bad_ap)
        refused_then_right(1, "volume mode", grp[0].probe_compose_advect, handles[0], bad_ap, [])
        refused_then_right(1, "exponent -65", ffi.group_probe_advect, grp, p, handles, probes._advect_params(0.001, exponents=[-65, 3]))
        # every dt and min_weight refusal of sph_probe_advect
        for mw in (0.0, -0.5, float("nan"), float("inf")):
            refused(1, "min_weight must be finite and > 0", probes.advect_group, grp, sets, P, 0.001, min_weight=mw)
            refused(1, "min_weight must be finite and > 0", grp[0].probe_compose_advect, handles[0], probes._advect_params(0.001, min_weight=mw, exponents=[3, 3]), [])
        for dt in (float("nan"), float("inf"), -float("inf")):
            refused(1, "dt must be finite", probes.advect_group, grp, sets, P, dt)
            refused(1, "dt must be finite", grp[0].probe_compose_advect, handles[0], probes._advect_params(dt, exponents=[3, 3]), [])
        still_right()
        # short buffers, by a byte
        need = 2 * n
        values, words_buf, info = np.empty(need, np.float32), np.empty(need, np.int64), ffi.SphProbeInfo()
        hc = (C.c_void_p * 2)(*[c.handle for c in grp])
        hs = (C.c_void_p * 2)(*handles)
        for vb, rb, what in [(need * 4 - 1, need * 8, "probe: output buffer"), (need * 4, need * 8 - 1, "raw output buffer")]:
            assert lib.group_probe_sample(hc, 2, C.byref(p), hs, C.byref(pp1), values.ctypes.data, vb, words_buf.ctypes.data, rb, C.byref(info)) == 1
            assert what in lib.last_error(grp[0].handle).decode()
            assert lib.probe_compose(plain.handle, plain_set.handle, C.byref(pp1), 0, None, None, None, values.ctypes.data, vb, words_buf.ctypes.data, rb, None) == 1
            assert what in lib.last_error(plain.handle).decode()
        assert lib.group_probe_sample(hc, 2, C.byref(p), hs, C.byref(pp1), None, need * 4, None, 0, None) == 1
        assert lib.group_probe_sample(hc, 2, C.byref(p), hs, C.byref(pp1), values.ctypes.data, need * 4, None, 0, None) == 0
        # handles that are no live set of the context they are used with
        refused_then_right(1, "not a live probe set of this context", grp[0].slab_probe_layer, p, handles[1], pp1)
        refused_then_right(1, "not a live probe set of this context", grp[0].slab_probe_layer_download, handles[1])
        refused_then_right(1, "not a live probe set of this context", grp[0].probe_compose, plain_set.handle, pp1, n, [])
        refused_then_right(1, "not a live probe set of this context", plain.probe_compose_advect, handles[0], ap, [])
        refused_then_right(1, "not a live probe set of this context", ffi.group_probe_sample, grp, p, handles[::-1], pp1, n)
        refused_then_right(1, "not a live probe set of this context", ffi.group_probe_advect, grp, p, [handles[0], None], ap)
        gone = probes.ProbeSet(grp[0], pts)
        dead = gone.handle
        gone.close()
        refused_then_right(1, "not a live probe set of this context", grp[0].slab_probe_layer, p, dead, pp1)
        # sets of different sizes in a group call
        short = probes.ProbeSet(grp[1], pts[:-1])
        refused_then_right(1, "set 1 holds", ffi.group_probe_sample, grp, p, [handles[0], short.handle], pp1, n)
        refused_then_right(1, "set 1 holds", ffi.group_probe_advect, grp, p, [handles[0], short.handle], ap)
        short.close()
        # n < 1, no members
        refused(1, "n < 1", ffi.group_probe_sample, [], p, [], pp1, n)
        refused(1, "n < 1", ffi.group_probe_advect, [], p, [], ap)
        assert lib.group_probe_sample(hc, 0, C.byref(p), hs, C.byref(pp1), values.ctypes.data, need * 4, None, 0, None) == 1
        assert lib.group_probe_advect(None, 2, C.byref(p), hs, C.byref(ap), None) == 1
        # a download with a capacity one entry short, or without its buffers
        info = grp[0].slab_probe_layer(p, handles[0], ppx)
        ne = int(info.n_entries)
        idx, wds = np.empty(ne, np.uint32), np.empty((len(names) + 1, ne), np.int64)
        assert lib.slab_probe_layer_download(grp[0].handle, handles[0], idx.ctypes.data, wds.ctypes.data, ne - 1) == 1
        assert "capacity" in lib.last_error(grp[0].handle).decode()
        assert lib.slab_probe_layer_download(grp[0].handle, handles[0], None, wds.ctypes.data, ne) == 1
        assert lib.slab_probe_layer_download(grp[0].handle, handles[0], idx.ctypes.data, wds.ctypes.data, ne) == 0
        assert np.array_equal(idx, good[0][0]) and np.array_equal(wds, good[0][1])
        # malformed layers are refused on the host, naming the layer, before anything is added: descending, repeated, >= n_points, NULL
        gi, gw = good[1]
        for bad_idx, word in ((gi[::-1].copy(), "layer 1.*not strictly ascending"), (np.concatenate([gi[:2], gi[1:-1]]), "layer 1.*not strictly ascending"),
                              (np.concatenate([gi[:-1], [n]]).astype(np.uint32), rf"layer 1.*point {n}, the set holds {n} points"),
                              (np.concatenate([gi[:-1], [0xFFFFFFFF]]).astype(np.uint32), "layer 1.*the set holds")):
            assert len(bad_idx) == len(gi)
            refused_then_right(1, word, grp[0].probe_compose, handles[0], ppx, n, [good[0], (bad_idx, gw)])
            refused_then_right(1, word, plain.probe_compose, plain_set.handle, ppx, n, [good[0], (bad_idx, gw)])
            refused_then_right(1, word, grp[1].probe_compose_advect, handles[1], ap, [(good[0][0], good[0][1][:3]), (bad_idx, gw[:3])])
        ne_arr = (C.c_uint64 * 2)(len(good[0][0]), len(gi))
        pi = (C.c_void_p * 2)(good[0][0].ctypes.data, None)
        pw = (C.c_void_p * 2)(good[0][1].ctypes.data, gw.ctypes.data)   # (4 planes each: room for compose's 4 and the advect's 3)
        big = np.empty((len(names) + 1) * n, np.float32)
        assert lib.probe_compose(grp[0].handle, handles[0], C.byref(ppx), 2, ne_arr, pi, pw, big.ctypes.data, big.nbytes, None, 0, None) == 1
        assert "layer 1 is NULL" in lib.last_error(grp[0].handle).decode()
        assert lib.probe_compose_advect(grp[0].handle, handles[0], C.byref(ap), 2, ne_arr, pi, pw, None) == 1
        assert "layer 1 is NULL" in lib.last_error(grp[0].handle).decode()
        assert lib.probe_compose(grp[0].handle, handles[0], C.byref(ppx), -1, None, None, None, big.ctypes.data, big.nbytes, None, 0, None) == 1
        assert lib.probe_compose(grp[0].handle, handles[0], C.byref(ppx), 2, None, pi, pw, big.ctypes.data, big.nbytes, None, 0, None) == 1
        assert "entry counts" in lib.last_error(grp[0].handle).decode()
        still_right()
        ffi.group_step(grp, p)   # the refusals left the group able to step, to sample and to move its tracers
        assert probes.sample_group(grp, sets, P, ch).weight.any() and probes.advect_group(grp, sets, P, 0.001).n_moved > 0
        assert np.array_equal(sets[0].points(), sets[1].points()) and not np.array_equal(sets[0].points(), pts)
    finally:
        plain.close()
        close_all(grp)


def test_a_poisoned_slab_group_is_not_probed(product_lib):
    """Contexts with room for their owned particles but not for a ghost layer: the step ends in SPH_ERR_CAPACITY and leaves them
    poisoned (tests/test_gpu_slab_sample.py); the range, the layer and the group calls answer SPH_ERR_POISONED."""
    from adaptive_sph_amd.workloads import dam_break_params
    scn = sc.dam_break_small(96, 48, 1 / 48)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    P = dam_break_params(max_iters=3, level_estimation_method="EmptyAngle", maximum_surface_distance=0.2, particle_radius_fine=0.004,
                         particle_radius_base=0.02)
    p = P.to_ffi()
    cuts = D.slab_cuts(pos[:, 0], 2)
    parts = D.partition(pos[:, 0], cuts)
    pp = _pp(["density"], [11])
    grp = []

    def refused(match, fn, *a):
        with pytest.raises(ffi.SphError, match=match) as e:
            fn(*a)
        assert e.value.status == 31, e.value

    try:
        for r in range(2):
            c = ffi.Context(product_lib, len(parts[r]) + 8, planes)
            c.dist_configure(r, 2, cuts[r], cuts[r + 1])
            c.upload(mass[parts[r]], pos[parts[r]], vel[parts[r]])
            c.upload_field("particle_id", parts[r].astype(np.uint32))
            grp.append(c)
        sets = [probes.ProbeSet(c, pos[::50]) for c in grp]
        handles = [s.handle for s in sets]
        with pytest.raises(ffi.SphError) as e:
            for _ in range(3):
                ffi.group_step(grp, p)
        assert e.value.status == 3
        refused("undefined", ffi.group_probe_sample, grp, p, handles, pp, len(sets[0]))
        refused("undefined", ffi.group_probe_advect, grp, p, handles, probes._advect_params(0.001))
        for c, h in zip(grp, handles):
            refused("undefined", c.slab_probe_range, p, pp)
            refused("undefined", c.slab_probe_layer, p, h, pp)
    finally:
        close_all(grp)
