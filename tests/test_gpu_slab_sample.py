"""Fields sampled from slab contexts (include/sph_slab_sample.h) against the numpy restatement of the sampling (tests/sample_reference.py,
tests/slab_sample_reference.py), bit for bit: the ranks' bands and layers word for word, the composed planes through the group call and
through the per-rank calls, that the ranks agree on the exponents and on the refusal, the row passes under a band offset, empty and
tiny grids, that a sample changes no state, and the refusals.

The expectation is always numpy fed with the GROUP's own fields assembled by global id -- never a plain context stepped beside it:
slab and plain runs need not agree bit for bit under the FAST policy."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

from adaptive_sph_amd import distributed as D, ffi, sampling, scene as sc
from adaptive_sph_amd.workloads import dam_break_params, default_params
from tests import sample_reference as sr, slab_sample_reference as ssr
from tests.test_gpu_slab_render import FIELDS, Group, _scene_a, _scene_b, close_all

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
CH = ["density", "pressure", "velocity_x", "velocity_y", "level_estimation"]   # tests/test_gpu_sample.py's
FIXTURES = ["A2", "A3", "B2", "B3"]


@pytest.fixture(scope="module")
def groups(product_lib):
    """which -> the loopback group of tests/test_gpu_slab_render.py's fixture (scene A: the 40 x 32 dam break with level estimation,
    4 steps; scene B: the 2:1 media scene with FromDistributionClamped1, 3 steps; k = 2 or 3 slabs, cuts through the fluid), built
    on first use, gathered once and left unchanged."""
    made = {}

    def get(which):
        if which not in made:
            g = (_scene_a if which[0] == "A" else _scene_b)(product_lib, int(which[1]))
            made[which] = g
            # cuts that run through the fluid: every rank owns particles; the device (slot) order is not the id order
            assert all(len(i) > 0 for i in g.ids)
            assert any(np.any(np.diff(i.astype(np.int64)) < 0) for i in g.ids), "slot order equals id order: the test would not see a mix-up"
            g.boundary = (sc.dam_break_small(40, 32, 1.0 / 40) if which[0] == "A" else
                          sc.SceneConfig.from_yaml(str(GOLDEN / "media" / "scene-ratio2to1.yaml"))).boundary
            g.own = [np.sort(i).astype(np.int64) for i in g.ids]
            g.twins = {}
        return made[which]

    yield get
    for g in made.values():
        g.close()


def _over_box(boundary, spacing, overhang=3):
    """A grid that overhangs the boundary box by `overhang` samples (and a fraction of one) on every side."""
    nx, ny = math.ceil(boundary.width / spacing) + 2 * overhang + 1, math.ceil(boundary.height / spacing) + 2 * overhang + 1
    return sampling.GridSpec(nx, ny, (-0.5 * boundary.width - (overhang + 0.3) * spacing, -0.5 * boundary.height - (overhang + 0.6) * spacing), spacing)


def _coarse_grid(g):
    """One support radius of the finest particle per sample (about 0.05 for scene A): the brute-force twin stays quick."""
    return _over_box(g.boundary, 2.0 * float(g.f["h2"].min()))


def _inner_grid(g):
    """The same spacing over the fluid's bounding box drawn in by 0.1 on every side: boxes are clipped at all four ends of the grid."""
    lo, hi = g.f["position"].min(axis=0) + 0.1, g.f["position"].max(axis=0) - 0.1
    spacing = 2.0 * float(g.f["h2"].min())
    return sampling.GridSpec(int((hi[0] - lo[0]) / spacing), int((hi[1] - lo[1]) / spacing), (float(lo[0]), float(lo[1])), spacing)


def _particles(g, channels=CH, volume="density"):
    return sr.Particles(g.f, channels, g.P.rest_density, g.P.maximum_surface_distance, volume)


def _twin(g, grid, channels=CH, volume="density", exps=None):
    """The twin over the whole vector and over every rank's owned particles, computed once per (grid, channels, volume, exponents):
    {"exps", "whole": (raw, footprints), "rank": [(raw, footprints, band)]}"""
    key = (grid, tuple(channels), volume, None if exps is None else tuple(exps))
    if key not in g.twins:
        tw = _particles(g, channels, volume)
        used = sr.exponents(tw) if exps is None else list(exps)
        X, Y = sr.centers(grid.nx, grid.ny, grid.origin, grid.spacing)
        ranks = []
        for own in g.own:
            sub = tw.subset(own)
            ranks.append(sr.raw_planes(sub, used, X, Y) + (ssr.band(sub.x, sub.y, sub.h, grid.nx, grid.ny, grid.origin, grid.spacing),))
        g.twins[key] = {"exps": used, "whole": sr.raw_planes(tw, used, X, Y), "rank": ranks}
    return g.twins[key]


def _sp(grid, channels, exps=None, **kw):
    return sampling.sample_params(grid, sampling.expand_channels(channels), exponents=exps, **kw)


def _rank_path(g, grid, channels=CH, exps=None, on=None, order=None, **kw):
    """The per-rank calls on every member, the fold, the compose on `on` (default: member 0) -> (raw, values, folded sp, bands, layers, infos)"""
    sp = _sp(grid, channels, exps, **kw)
    words = [c.slab_sample_range(g.p, sp) for c in g.ctxs]
    sp = ffi.sample_fold_words(g.ctxs[0].lib, words, sp)
    bands, layers, infos = [], [], []
    for c in g.ctxs:
        b, info = c.slab_sample_layer(g.p, sp)
        bands.append(b)
        infos.append(info)
        layers.append(c.slab_sample_layer_download() if b.sx1 > b.sx0 else None)
    order = list(range(len(bands))) if order is None else order
    values, raw = (on or g.ctxs[0]).sample_compose(sp, [bands[i] for i in order], [layers[i] for i in order], raw=True)
    return raw, values, sp, bands, layers, infos


def _group_path(g, grid, channels=CH, **kw):
    out = sampling.sample_group(g.ctxs, g.P, grid, channels, raw=True, **kw)
    names = ["weight"] + sampling.expand_channels(channels)
    return np.stack([out.raw[k] for k in names]), np.stack([out.planes[k] for k in names]), out


def _diff(a, b):
    return [int(np.count_nonzero(a[k] != b[k])) for k in range(len(a))]


# ---- 1. layers word for word -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("volume", ["density", "rest"])
@pytest.mark.parametrize("which", FIXTURES)
def test_layers_word_for_word(groups, which, volume):
    g = groups(which)
    _layers_word_for_word(g, which, volume, _coarse_grid(g), overhang=True)
    if volume == "density":
        _layers_word_for_word(g, which, volume, _inner_grid(g), overhang=False)


def _layers_word_for_word(g, which, volume, grid, overhang):
    tw = _twin(g, grid, CH, volume)
    sp = _sp(grid, CH, tw["exps"], volume=volume)
    pairs, touching = 0, 0
    for r, c in enumerate(g.ctxs):
        want, foot, want_band = tw["rank"][r]
        band, info = c.slab_sample_layer(g.p, sp)
        print(which, volume, "rank", r, "band", band.as_tuple(), "twin", want_band, "pairs", int(info.n_pairs), int(foot.sum()))
        assert band.as_tuple() == want_band and band.sx1 > band.sx0
        assert band.n_boxes == len(g.own[r]) if overhang else 0 < band.n_boxes <= len(g.own[r])
        layer = c.slab_sample_layer_download()
        assert layer.dtype == np.int64 and layer.shape == (len(CH) + 1, grid.ny, band.sx1 - band.sx0)
        full = np.zeros((len(CH) + 1, grid.ny, grid.nx), np.int64)
        full[:, :, band.sx0:band.sx1] = layer
        assert np.array_equal(full, want), (which, volume, r, _diff(full, want))
        assert want[0].any() and not want[:, :, :band.sx0].any() and not want[:, :, band.sx1:].any()
        assert list(info.exponents)[:len(CH)] == tw["exps"]
        assert (int(info.n_touching), int(info.max_footprint), int(info.n_pairs)) == (int((foot > 0).sum()), int(foot.max()), int(foot.sum()))
        pairs += int(info.n_pairs)
        touching += int(info.n_touching)
    whole_foot = tw["whole"][1]
    assert pairs == int(whole_foot.sum()) and touching == int((whole_foot > 0).sum())
    # adjacent bands overlap: the supports reach across the cut
    bands = [tw["rank"][r][2] for r in range(len(g.ctxs))]
    assert all(bands[r + 1][0] < bands[r][1] for r in range(len(bands) - 1)), bands
    if not overhang:   # the outer ranks' boxes are cut by the grid's first and last column, every rank's by its first and last row
        assert bands[0][0] == 0 and bands[-1][1] == grid.nx
        assert all(t[0][0, 0].any() and t[0][0, -1].any() for t in tw["rank"])
    # the layers add up to the whole vector's planes
    assert np.array_equal(sum(t[0] for t in tw["rank"]), tw["whole"][0])


# ---- 2. composed planes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("volume", ["density", "rest"])
@pytest.mark.parametrize("which", FIXTURES)
def test_composed_planes(groups, product_lib, which, volume):
    g = groups(which)
    grid = _coarse_grid(g)
    tw = _twin(g, grid, CH, volume)
    want, foot = tw["whole"]
    raw, values, out = _group_path(g, grid, CH, volume=volume)
    assert raw.shape == want.shape == (len(CH) + 1, grid.ny, grid.nx)
    assert np.array_equal(raw, want), (which, volume, "group", _diff(raw, want))
    assert list(out.exponents.values()) == tw["exps"]
    assert (out.n_touching, out.max_footprint, out.n_pairs) == (int((foot > 0).sum()), int(foot.max()), int(foot.sum()))
    assert np.array_equal(values.view(np.uint32), sampling.resolve(raw, tw["exps"]).view(np.uint32))
    held = sampling.sample_group(g.ctxs, g.P, grid, CH, volume=volume, raw=True, host=ffi.HostBuffers())     # into persistent host buffers
    assert np.array_equal(held.raw["velocity_y"], want[4]) and np.array_equal(held["weight"].view(np.uint32), values[0].view(np.uint32))
    # the group call leaves every member's layer as the layer call does
    for r, c in enumerate(g.ctxs):
        b = tw["rank"][r][2]
        assert product_lib.slab_sample_layer_download(c.handle, None, 0) == 1 and "capacity" in product_lib.last_error(c.handle).decode()
        layer = np.empty((len(CH) + 1, grid.ny, b[1] - b[0]), np.int64)
        assert product_lib.slab_sample_layer_download(c.handle, layer.ctypes.data, layer.size) == 0
        assert np.array_equal(layer, tw["rank"][r][0][:, :, b[0]:b[1]])
    # the per-rank calls, folded and composed: on member 0, in reversed order on the last member, on a fresh plain context
    raw2, values2, sp, bands, layers, _ = _rank_path(g, grid, CH, volume=volume)
    assert np.array_equal(raw2, want), (which, volume, "per rank", _diff(raw2, want))
    assert [sp.channels[k].exponent for k in range(len(CH))] == tw["exps"]
    assert np.array_equal(values2.view(np.uint32), values.view(np.uint32))
    back = list(range(len(bands)))[::-1]
    assert np.array_equal(g.ctxs[-1].sample_compose(sp, [bands[i] for i in back], [layers[i] for i in back], raw=True)[1], want)
    plain = ffi.Context(product_lib, 16, g.planes)
    try:
        assert np.array_equal(plain.sample_compose(sp, bands, layers, raw=True)[1], want)
    finally:
        plain.close()


@pytest.mark.parametrize("which", ["A3", "B2"])
def test_resolved_planes_with_normalise_and_fill(groups, which):
    g = groups(which)
    grid = _coarse_grid(g)
    kw = dict(normalize=True, min_weight=0.5, fill=float("nan"))
    want_raw = _twin(g, grid)["whole"][0]
    raw_g, values_g, out = _group_path(g, grid, CH, **kw)
    raw_r, values_r, sp = _rank_path(g, grid, CH, **kw)[:3]
    for raw, values, exps in ((raw_g, values_g, list(out.exponents.values())), (raw_r, values_r, [sp.channels[k].exponent for k in range(len(CH))])):
        assert np.array_equal(raw, want_raw)
        want = sampling.resolve(raw, exps, **kw)
        nan = np.isnan(want)
        assert nan[1:].any() and (~nan[1:]).any() and not nan[0].any()               # min_weight has samples on both sides
        assert np.array_equal(np.isnan(values), nan)
        assert np.array_equal(values.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ---- 3. the ranks agree on the exponents -----------------------------------------------------------------------------------------
def test_ranks_agree_on_the_exponents(groups):
    """With automatic exponents the group takes exponent_of of the WHOLE vector's maxima; on some fixture and channel two ranks' own
    maxima give different exponents -- a rank that took its own would scatter at another scale."""
    differ = []
    for which in FIXTURES:
        g = groups(which)
        grid = _coarse_grid(g)
        tw = _particles(g)
        whole = [max(sr.exponent_of(m), -64) for m in sr.max_abs(tw)]
        sp = _sp(grid, CH)
        words = [c.slab_sample_range(g.p, sp) for c in g.ctxs]
        own = []
        for r, w in enumerate(words):
            want = ssr.words(tw.subset(g.own[r]), g.own[r])
            assert w.as_tuple() == want and w.first_bad == ffi.SAMPLE_NO_OFFENDER, (which, r)
            own.append(ssr.fold_words([w.as_tuple()], CH, [None] * len(CH))[1])
        print(which, "whole", whole, "ranks", own)
        folded = ffi.sample_fold_words(g.ctxs[0].lib, words, sp)
        assert [folded.channels[k].exponent for k in range(len(CH))] == whole == ssr.fold_words([w.as_tuple() for w in words], CH, [None] * len(CH))[1]
        assert list(sampling.sample_group(g.ctxs, g.P, grid, CH).exponents.values()) == whole
        differ += [(which, CH[k]) for k in range(len(CH)) if len({e[k] for e in own}) > 1]
    assert differ, "every rank's own maxima give the whole vector's exponents on every fixture: the test shows nothing"


# ---- 4. row passes under a band offset -------------------------------------------------------------------------------------------
def test_row_passes_under_a_band_offset(groups):
    g = groups("A2")
    ch = ["density", "velocity_x"]
    x = g.f["position"][:, 0]
    cut = 0.5 * (float(x[g.own[0]].max()) + float(x[g.own[1]].min()))
    near = np.argsort(np.abs(x - cut))[:40]
    mid = near[np.argsort(g.f["position"][near, 1])[len(near) // 2]]           # a particle at the cut, half way up the column
    h = float(g.f["h2"][mid])
    spacing = 2.0 * h / 104.0                                                  # a disc of radius 104 samples: about 34 000 of them
    grid = sampling.GridSpec(320, 320, (cut - 160 * spacing, float(g.f["position"][mid, 1]) - 160 * spacing), spacing)
    tw = _particles(g, ch)
    exps = sr.exponents(tw)
    want = sr.window_planes(tw, exps, grid.nx, grid.ny, grid.origin, grid.spacing, (0, grid.nx, 0, grid.ny))
    raw, _, out = _group_path(g, grid, ch)
    assert out.max_footprint > 32768
    assert np.array_equal(raw, want), _diff(raw, want)
    raw2, _, _, bands, layers, infos = _rank_path(g, grid, ch)
    assert np.array_equal(raw2, want), _diff(raw2, want)
    assert all(b.sx1 > b.sx0 for b in bands) and bands[1].sx0 > 0 and bands[0].sx1 < grid.nx, [b.as_tuple() for b in bands]
    assert max(int(i.max_footprint) for i in infos) == out.max_footprint and sum(int(i.n_pairs) for i in infos) == out.n_pairs
    for r in range(2):   # every rank's layer alone, against the windowed twin of its own particles
        full = np.zeros_like(want)
        full[:, :, bands[r].sx0:bands[r].sx1] = layers[r]
        assert np.array_equal(full, sr.window_planes(tw.subset(g.own[r]), exps, grid.nx, grid.ny, grid.origin, grid.spacing, (0, grid.nx, 0, grid.ny))), r


# ---- 5. empty and tiny -----------------------------------------------------------------------------------------------------------
def test_empty_and_tiny_grids(groups, product_lib):
    g = groups("A3")
    pos = g.f["position"]
    reach = 2.2 * float(g.f["h2"].max())
    # a grid that only rank 0's slab reaches: it ends more than a support radius (and the box's padding) left of rank 1's first particle
    x_end = float(pos[g.own[1], 0].min()) - reach - 0.08
    x_lo = float(pos[:, 0].min()) - 0.1
    spacing = 0.03
    only0 = sampling.GridSpec(int((x_end - x_lo) / spacing), 30, (x_lo, float(pos[:, 1].min()) - 0.1), spacing)
    assert only0.nx >= 4
    want = _twin(g, only0)["whole"][0]
    raw, _, sp, bands, layers, _ = _rank_path(g, only0)
    assert want[0].any() and np.array_equal(raw, want)
    assert bands[0].sx1 > bands[0].sx0 and all(b.as_tuple() == (0, 0, 0) for b in bands[1:]) and all(l is None for l in layers[1:])
    assert np.array_equal(_group_path(g, only0)[0], want)
    assert np.array_equal(_twin(g, only0)["rank"][0][0], want)
    # one sample, inside the fluid
    mid = 0.5 * (pos.min(axis=0) + pos.max(axis=0))
    one = sampling.GridSpec(1, 1, (float(mid[0]) - 0.01, float(mid[1]) - 0.01), 0.02)
    want = _twin(g, one)["whole"][0]
    assert want.shape == (len(CH) + 1, 1, 1) and want[0, 0, 0] > 0
    assert np.array_equal(_group_path(g, one)[0], want) and np.array_equal(_rank_path(g, one)[0], want)
    # beside the fluid (the right half of the box: nothing there after four steps): all zeros, no band anywhere
    beside = sampling.GridSpec(9, 7, (1.0, 0.3), 0.05)
    raw, values, out = _group_path(g, beside, normalize=True, fill=-7.5)
    assert not raw.any() and (out.n_touching, out.max_footprint, out.n_pairs) == (0, 0, 0)
    assert not values[0].any() and np.array_equal(values[1:], np.full(values[1:].shape, -7.5, np.float32))
    raw, _, sp, bands, layers, _ = _rank_path(g, beside)
    assert not raw.any() and all(b.as_tuple() == (0, 0, 0) for b in bands) and all(l is None for l in layers)
    for c in g.ctxs:   # an empty layer downloads as nothing, whatever the capacity
        assert product_lib.slab_sample_layer_download(c.handle, None, 0) == 0
    # no layers at all
    values, raw = g.ctxs[1].sample_compose(sp, [], [], raw=True)
    assert raw.shape == (len(CH) + 1, 7, 9) and not raw.any() and not values.any()


# ---- 6. one refusal on every path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["A2", "A3"])   # (scene B's columns stand still in x: no velocity_x to refuse)
def test_one_refusal_on_every_path(groups, which):
    g = groups(which)
    grid = _coarse_grid(g)
    tw = _particles(g)
    vx = np.abs(g.f["velocity"][:, 0])
    tops = sorted(float(vx[own].max()) for own in g.own)
    e = sr.exponent_of(tops[-2]) - 1                     # 2^e <= the second largest of the ranks' maxima: two ranks reach it
    assert sum(bool((vx[own] >= 2.0 ** e).any()) for own in g.own) >= 2
    exps = [None, None, e, None, None]
    idx, why = sr.first_offender(tw, exps)
    assert why == sr.BAD_CHANNEL + 2
    kind, sentence = ssr.fold_words([ssr.words(tw.subset(own), own, exps) for own in g.own], CH, exps)
    assert kind == "refused" and f"(particle i={idx})" in sentence and "channel 2 (velocity) is not finite or not below 2^exponent" in sentence
    ranks_first = [ssr.words(tw.subset(own), own, exps)[0] for own in g.own]
    assert sum(f != ssr.NONE for f in ranks_first) >= 2 and len(set(ranks_first)) == len(ranks_first)
    with pytest.raises(ffi.SphError) as err:
        sampling.sample_group(g.ctxs, g.P, grid, CH, exponents=exps)
    assert err.value.status == 1 and sentence in str(err.value), (err.value, sentence)
    sp = _sp(grid, CH, exps)
    words = [c.slab_sample_range(g.p, sp) for c in g.ctxs]
    assert [w.first_bad for w in words] == ranks_first
    for order in (words, words[::-1]):
        with pytest.raises(ffi.SphError) as err:
            ffi.sample_fold_words(g.ctxs[0].lib, order, sp)
        assert err.value.status == 1 and str(err.value).endswith(sentence), (err.value, sentence)
    # nothing changed: the next sample is the twin's
    assert np.array_equal(_group_path(g, grid)[0], _twin(g, grid)["whole"][0])


def test_refused_before_the_first_step_then_steps_on(product_lib):
    P = default_params(merging=False, sharing=False, splitting=False, max_dt=0.004, maximum_surface_distance=0.2)
    scn = sc.dam_break_small(24, 20, 1.0 / 24)
    pos, mass, vel = sc.init_particles(scn)
    g = Group.__new__(Group)                              # (Group gathers the outputs of a step: this one has not stepped yet)
    g.P, g.p, g.n, g.planes = P, P.to_ffi(), len(mass), sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    g.ctxs = D.make_loopback_group(product_lib, pos, mass, vel, g.planes, 2)   # no step yet: h is 0, every slot is owned
    try:
        grid = sampling.GridSpec(57, 43, (-2.05, -1.04), 0.021)
        with pytest.raises(ffi.SphError, match=r"particle i=0; before the first step") as err:
            sampling.sample_group(g.ctxs, g.P, grid, CH)
        assert err.value.status == 1
        sp = _sp(grid, CH)
        words = [c.slab_sample_range(g.p, sp) for c in g.ctxs]
        assert min(w.first_bad for w in words) == sr.BAD_H and all(w.first_bad & 0xFF == sr.BAD_H for w in words)
        assert len({w.first_bad for w in words}) == 2     # every rank names the smallest id it owns
        with pytest.raises(ffi.SphError, match=r"particle i=0; before the first step") as err:
            ffi.sample_fold_words(product_lib, words, sp)
        assert err.value.status == 1
        for _ in range(2):                                # not poisoned: the group steps on, and the sample is the twin's
            ffi.group_step(g.ctxs, g.p)
        g.gather()
        g.own = [np.sort(i).astype(np.int64) for i in g.ids]
        g.twins = {}
        want = _twin(g, grid)["whole"][0]
        assert want[0].any() and np.array_equal(_group_path(g, grid)[0], want) and np.array_equal(_rank_path(g, grid)[0], want)
    finally:
        g.close()


# ---- 7. a sample changes no state ------------------------------------------------------------------------------------------------
def test_a_sample_changes_no_state(product_lib):
    """Two identical 2-slab groups; one is sampled through the group call and through the per-rank calls; then both step twice: every
    downloadable field, the ids and the exported lists are equal byte for byte."""
    P = default_params(merging=False, sharing=False, splitting=False, max_dt=0.004, maximum_surface_distance=0.2)
    scn = sc.dam_break_small(32, 32, 1.0 / 32)
    a = Group(product_lib, scn, P, 2, 2)
    b = Group(product_lib, scn, P, 2, 2)
    try:
        grid = sampling.GridSpec(160, 90, (-2.0, -1.0), 0.0125)
        for volume, normalize in (("density", False), ("rest", True)):
            assert sampling.sample_group(a.ctxs, P, grid, CH, volume=volume, normalize=normalize)["weight"].any()
            assert _rank_path(a, grid, CH, volume=volume, normalize=normalize)[0].any()
        for _ in range(2):
            ffi.group_step(a.ctxs, a.p)
            ffi.group_step(b.ctxs, b.p)
        for x, y in zip(a.ctxs, b.ctxs):
            for f in FIELDS + ["particle_id", "cell_index", "h2_next", "level_old", "lambda_sum"]:
                assert x.download(f).tobytes() == y.download(f).tobytes(), f
            (oa, ia), (ob, ib) = x.download_neighbors(), y.download_neighbors()
            assert np.array_equal(oa, ob) and np.array_equal(ia, ib)
        # a layer is a read-out: it outlives the steps
        assert a.ctxs[0].slab_sample_layer_download().any()
    finally:
        a.close()
        b.close()


# ---- 8. argument refusals --------------------------------------------------------------------------------------------------------
def _refused(status, word, f, *a, **kw):
    with pytest.raises(ffi.SphError) as e:
        f(*a, **kw)
    assert e.value.status == status and word in str(e.value), (status, word, e.value)


def test_refusals(product_lib):
    P = default_params(merging=False, sharing=False, splitting=False, max_dt=0.004)
    scn = sc.dam_break_small(32, 32, 1.0 / 32)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    p = P.to_ffi()
    plain = ffi.Context(product_lib, len(mass) + 64, planes)
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 2)
    grid = sampling.GridSpec(40, 30, (-2.0, -1.0), 0.05)
    sp = _sp(grid, ["density"], [1])
    sp_auto = _sp(grid, ["density"])
    try:
        plain.upload(mass, pos, vel)
        # the per-rank calls on a plain context, a plain context as a member; sph_sample_grid on a slab context still refuses
        _refused(30, "sph_sample_grid samples a plain context", plain.slab_sample_range, p, sp)
        _refused(30, "sph_sample_grid samples a plain context", plain.slab_sample_layer, p, sp)
        _refused(30, "sph_sample_grid samples a plain context", plain.slab_sample_layer_download)
        _refused(30, "sph_sample_grid samples a plain context", ffi.group_sample_grid, [grp[0], plain], p, sp)
        _refused(30, "sph_sample_grid samples a plain context", ffi.group_sample_grid, [plain, grp[0]], p, sp)
        _refused(30, "one rank holds a slab", sampling.sample_grid, grp[0], P, grid, ["density"])
        # a download before any layer
        _refused(1, "no layer", grp[0].slab_sample_layer_download)
        ffi.group_step(grp, p)
        # an automatic exponent given to the layer call and to compose
        _refused(1, "sph_sample_fold_words", grp[0].slab_sample_layer, p, sp_auto)
        _refused(1, "sph_sample_fold_words", plain.sample_compose, sp_auto, [], [])
        _refused(1, "no layer", grp[0].slab_sample_layer_download)              # (a refused layer call leaves none)
        # null arguments
        _refused(1, "null", grp[0].slab_sample_range, None, sp)
        _refused(1, "null", grp[0].slab_sample_range, p, None)
        _refused(1, "null", grp[0].slab_sample_layer, p, None)
        _refused(1, "null", ffi.group_sample_grid, grp, None, sp)
        _refused(1, "null", ffi.group_sample_grid, grp, p, None)
        assert product_lib.slab_sample_range(grp[0].handle, C.byref(p), C.byref(sp), None) == 1
        assert product_lib.slab_sample_layer(grp[0].handle, C.byref(p), C.byref(sp), None, None) == 1
        # the geometry, channel and buffer refusals of sph_sample_grid, once each, on the group call (and the per-rank calls)
        cases = [(sampling.GridSpec(0, 30, (-2.0, -1.0), 0.05), "per side"), (sampling.GridSpec(40, 16385, (-2.0, -1.0), 0.05), "per side"),
                 (sampling.GridSpec(16384, 16384, (-2.0, -1.0), 0.05), "at most"), (sampling.GridSpec(40, 30, (-2.0, -1.0), 0.0), "spacing"),
                 (sampling.GridSpec(40, 30, (-2.0, -1.0), float("nan")), "spacing"), (sampling.GridSpec(40, 30, (float("inf"), 0.0), 0.05), "origin")]
        bad = [(_sp(gr, ["density"], [1]), word) for gr, word in cases]
        q = _sp(grid, ["density"] * 6, [1] * 6)
        q.n_channels = 7
        bad.append((q, "7 channels"))
        q = _sp(grid, ["density", "pressure"], [1, 1])
        q.channels[1].field = ffi.FIELDS["mass"][0]
        bad.append((q, "cannot be sampled"))
        q = _sp(grid, ["density", "pressure"], [1, 1])
        q.channels[1].component = 1
        bad.append((q, "pressure has no component 1"))
        q = _sp(grid, ["density"], [65])
        bad.append((q, "exponent 65"))
        q = _sp(grid, ["density"], [1])
        q.volume = 2
        bad.append((q, "volume mode"))
        for q, word in bad:
            _refused(1, word, ffi.group_sample_grid, grp, p, q)
            _refused(1, word, grp[1].slab_sample_range, p, q)
            _refused(1, word, grp[1].slab_sample_layer, p, q)
            _refused(1, word, plain.sample_compose, q, [], [])
        need = 2 * 40 * 30
        values, raw_buf, info = np.empty(need, np.float32), np.empty(need, np.int64), ffi.SphSampleInfo()
        handles = (C.c_void_p * 2)(*[c.handle for c in grp])
        for vb, rb, what in [(need * 4 - 1, need * 8, "sample: output buffer"), (need * 4, need * 8 - 1, "raw output buffer")]:   # short by a byte
            assert product_lib.group_sample_grid(handles, 2, C.byref(p), C.byref(sp), values.ctypes.data, vb, raw_buf.ctypes.data, rb, C.byref(info)) == 1
            assert what in product_lib.last_error(grp[0].handle).decode()
            assert product_lib.sample_compose(plain.handle, C.byref(sp), 0, None, None, values.ctypes.data, vb, raw_buf.ctypes.data, rb) == 1
            assert what in product_lib.last_error(plain.handle).decode()
        assert product_lib.group_sample_grid(handles, 2, C.byref(p), C.byref(sp), None, need * 4, None, 0, None) == 1           # no output buffer at all
        assert product_lib.group_sample_grid(handles, 2, C.byref(p), C.byref(sp), values.ctypes.data, need * 4, None, 0, None) == 0
        # n = 0, no members
        _refused(1, "n < 1", ffi.group_sample_grid, [], p, sp)
        assert product_lib.group_sample_grid(handles, 0, C.byref(p), C.byref(sp), values.ctypes.data, need * 4, None, 0, None) == 1
        assert product_lib.group_sample_grid(None, 2, C.byref(p), C.byref(sp), values.ctypes.data, need * 4, None, 0, None) == 1
        # a layer, then a capacity one word short
        band, _ = grp[0].slab_sample_layer(p, sp)
        n_words = 2 * 30 * (band.sx1 - band.sx0)
        assert n_words > 1
        short = np.empty(n_words - 1, np.int64)
        assert product_lib.slab_sample_layer_download(grp[0].handle, short.ctypes.data, short.size) == 1
        assert "capacity" in product_lib.last_error(grp[0].handle).decode()
        assert product_lib.slab_sample_layer_download(grp[0].handle, None, n_words) == 1
        layer = grp[0].slab_sample_layer_download()
        # bands that are no column range of the grid; a NULL layer for a band that is not empty; layers without their bands
        B = ffi.SphSampleBand
        for b in (B(3, 2, 0, 0), B(-1, 4, 0, 0), B(0, 41, 0, 0), B(41, 41, 0, 0)):
            _refused(1, "band", plain.sample_compose, sp, [b], [np.zeros((2, 30, max(b.sx1 - b.sx0, 0)), np.int64)])
        _refused(1, "NULL", plain.sample_compose, sp, [band], [None])
        assert product_lib.sample_compose(plain.handle, C.byref(sp), -1, None, None, values.ctypes.data, need * 4, None, 0) == 1
        assert product_lib.sample_compose(plain.handle, C.byref(sp), 1, None, None, values.ctypes.data, need * 4, None, 0) == 1
        assert "bands" in product_lib.last_error(plain.handle).decode()
        _, raw = plain.sample_compose(sp, [band, B(40, 40, 0, 0)], [layer, None], raw=True)
        assert np.array_equal(raw[:, :, band.sx0:band.sx1], layer) and not raw[:, :, band.sx1:].any()
        ffi.group_step(grp, p)   # the refusals left the group able to step and to sample
        assert ffi.group_sample_grid(grp, p, sp_auto, raw=True)[1][0].any()
    finally:
        plain.close()
        close_all(grp)


def test_a_poisoned_slab_group_is_not_sampled(product_lib):
    """Contexts with room for their owned particles but not for a ghost layer: the step ends in SPH_ERR_CAPACITY and leaves them
    poisoned (tests/test_gpu_slab_render.py); the range, the layer and the group call answer SPH_ERR_POISONED."""
    scn = sc.dam_break_small(96, 48, 1 / 48)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    P = dam_break_params(max_iters=3, level_estimation_method="EmptyAngle", maximum_surface_distance=0.2, particle_radius_fine=0.004,
                         particle_radius_base=0.02)
    p = P.to_ffi()
    cuts = D.slab_cuts(pos[:, 0], 2)
    parts = D.partition(pos[:, 0], cuts)
    sp = _sp(sampling.GridSpec(40, 30, (-2.0, -1.0), 0.05), ["density"], [1])
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
        _refused(31, "undefined", ffi.group_sample_grid, grp, p, sp)
        for c in grp:
            _refused(31, "undefined", c.slab_sample_range, p, sp)
            _refused(31, "undefined", c.slab_sample_layer, p, sp)
    finally:
        close_all(grp)
