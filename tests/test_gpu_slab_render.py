"""Frames drawn from slab contexts (include/sph_slab_render.h) against the numpy restatement of the renderer (tests/render_reference.py),
byte for byte: the ranks' layers word for word, the composed frame through the group call and through the per-rank calls, against
sph_render of a plain context holding the same particles, that drawing changes no state, and the refusals.

The expectation is always numpy fed with the GROUP's own fields assembled by global id -- never a plain context stepped beside it:
slab and plain runs need not agree bit for bit under the FAST policy."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from adaptive_sph_amd import distributed as D, ffi, render, scene as sc
from adaptive_sph_amd.workloads import dam_break_params, default_params
from tests import render_reference as rr

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"
FIELDS = ["mass", "position", "velocity", "density", "aii", "constant_field", "ppe_source_term", "pressure", "level_estimation", "stash",
          "neighbor_count", "particle_size_class", "flag_is_fluid_surface", "flag_insufficient_neighs", "flag_neighborhood_reduced", "h2"]
ALL_FLAGS = ffi.RENDER_SHOW_SURFACE | ffi.RENDER_SHOW_NEIGHBORHOOD_REDUCED
COLOUR_VIEW = (160, 80, 2, 1.05)   # a supersampled view that holds every rank's slab (scene A stands at x in [-2, -1])
FRAMES = [("Velocity", 300, 200, 1, 1.04), ("RandomColor", 160, 250, 2, 0.9), ("NeighborCount", 257, 129, 2, 1.3),
          ("Pressure", 200, 200, 1, 1.0), ("MinDistanceToNeighbor", 128, 96, 1, 1.04)]


def _stops(P, attr):
    cm = render.get_color_map(attr, P)
    return [] if cm is None else [(float(v), *map(float, c)) for v, c in cm.color_stops()]


def _vis(attr, flags=0):
    return render.VisualizationParams(attr, show_flag_is_fluid_surface=bool(flags & ffi.RENDER_SHOW_SURFACE),
                                      show_flag_neighborhood_reduced=bool(flags & ffi.RENDER_SHOW_NEIGHBORHOOD_REDUCED),
                                      take_data_from_stash=bool(flags & ffi.RENDER_FROM_STASH))


def close_all(ctxs):
    for c in ctxs:
        c.close()


class Group:
    """A loopback group behind its steps + everything numpy needs of it, gathered ONCE by global id and left unchanged."""

    def __init__(self, lib, scn, P, k, steps, cut_choices=(None,), planes=None):
        pos, mass, vel = sc.init_particles(scn)
        self.P, self.p = P, P.to_ffi()
        self.planes = planes if planes is not None else sc.boundary_planes(scn.boundary, P.init_boundary_handler)
        self.n = len(mass)
        last = None
        for cuts in cut_choices:   # (a cut the group refuses as narrower than two ghost layers: the next choice)
            self.ctxs = D.make_loopback_group(lib, pos, mass, vel, self.planes, k, cuts=cuts)
            try:
                for _ in range(steps):
                    ffi.group_step(self.ctxs, self.p)
                last = None
                break
            except ffi.SphError as e:
                close_all(self.ctxs)
                last = e
                if e.status != 30:
                    raise
        if last is not None:
            raise last
        self.gather()

    def gather(self):
        self.ids = [c.download("particle_id") for c in self.ctxs]
        assert np.array_equal(np.sort(np.concatenate(self.ids)), np.arange(self.n))
        self.f = {f: D.gather_by_id(self.ctxs, f, self.n) for f in FIELDS}
        self.rad = rr.radii(self.f["mass"], self.P.rest_density)
        self.lists = None
        self._keys = {}

    def neighbors(self):
        if self.lists is None:
            off, idx = D.assemble_lists(self.ids, [c.download_neighbors() for c in self.ctxs], self.n)
            self.lists = (off, idx)
        return self.lists

    def colors(self, attr, flags=0):
        nb = self.neighbors() if attr == "MinDistanceToNeighbor" else None
        return rr.colors(self.f, attr, flags, _stops(self.P, attr), self.P.rest_density, self.P.maximum_surface_distance, nb)

    def frame(self, w, h, s, zoom):
        """-> (rr.Frame, its sample keys over the whole vector): the keys depend on the geometry alone, shared by every attribute"""
        key = (w, h, s, zoom)
        if key not in self._keys:
            fr = rr.Frame(w, h, s, zoom, render.boundary_segments(self.planes))
            self._keys[key] = (fr, fr.keys(self.f["position"], self.rad))
        return self._keys[key]

    def expected(self, attr, flags, w, h, s, zoom):
        fr, keys = self.frame(w, h, s, zoom)
        return fr.resolve(keys, self.f["position"], self.rad, self.colors(attr, flags))

    def rp(self, attr, flags, w, h, s, zoom):
        return render.render_params(_vis(attr, flags), self.P, w, h, s, zoom, render.boundary_segments(self.planes))

    def layers(self, attr, flags, w, h, s, zoom):
        """The three per-rank calls on every member -> (rp, bands, layers; None for an empty band)."""
        rp = self.rp(attr, flags, w, h, s, zoom)
        pmax = max(c.slab_render_pressure_max() for c in self.ctxs) if attr == "Pressure" else 0.0
        bands = [c.slab_render_layer(self.p, rp, pmax) for c in self.ctxs]
        layers = [c.slab_render_layer_download() if b.sx1 > b.sx0 else None for c, b in zip(self.ctxs, bands)]
        for b, l in zip(bands, layers):
            assert 0 <= b.sx0 <= b.sx1 <= w * s
            assert l is None or (l.shape == (h * s, b.sx1 - b.sx0) and l.dtype == np.uint64)
        return rp, bands, layers

    def group_frame(self, attr, flags, w, h, s, zoom):
        return render.render_group(self.ctxs, self.P, _vis(attr, flags), w, h, s, zoom, self.planes)

    def expected_layer(self, r, attr, flags, w, h, s, zoom):
        """uint64[HS, WS]: rank r's words over the WHOLE sample grid, from rr.Frame.keys over the particles it owns in id order (the
        largest local index is then the largest id), the fill test of rr.Frame.resolve and the colours of the whole vector."""
        fr, _ = self.frame(w, h, s, zoom)
        own = np.sort(self.ids[r]).astype(np.int64)
        pos, rad = self.f["position"][own], self.rad[own]
        k = fr.keys(pos, rad).astype(np.int64)
        px, py, _, ri = fr.discs(pos, rad)
        sy, sx = np.mgrid[0:fr.hs, 0:fr.ws]
        cov = k > 0
        wl = k[cov] - 1
        du = (sx[cov].astype(rr.f32) + rr.f32(0.5)) - px[wl]
        dv = (sy[cov].astype(rr.f32) + rr.f32(0.5)) - py[wl]
        fill = du * du + dv * dv < ri[wl] * ri[wl]
        rgb = self.colors(attr, flags).astype(np.uint64)[own[wl]]
        rgb24 = np.where(fill, rgb[:, 0] | (rgb[:, 1] << np.uint64(8)) | (rgb[:, 2] << np.uint64(16)), np.uint64(0))
        out = np.zeros((fr.hs, fr.ws), np.uint64)
        out[cov] = ((own[wl].astype(np.uint64) + np.uint64(1)) << np.uint64(32)) | rgb24
        return out

    def close(self):
        close_all(self.ctxs)


def _scene_a(lib, k):
    """A small dam break, level estimation and the neighbourhood constraint on (every flag can be set), 4 group steps."""
    P = default_params(merging=False, sharing=False, splitting=False, constrain_neighborhood_count=True, max_dt=0.004, maximum_surface_distance=0.2)
    return Group(lib, sc.dam_break_small(40, 32, 1.0 / 40), P, k, 4, [None] + ([[-D.INF, -1.66, -1.30, D.INF], [-D.INF, -1.70, -1.25, D.INF]] if k == 3 else []))


def _scene_b(lib, k):
    """The media recipes' 2:1 scene (two block spacings) with the distribution-based smoothing length, 3 group steps.  Three slabs: one
    cut through the fine block, one through the coarse block (equal counts would put both into the fine one, 0.2 apart)."""
    scn = sc.SceneConfig.from_yaml(str(GOLDEN / "media" / "scene-ratio2to1.yaml"))
    P = default_params(merging=False, sharing=False, splitting=False, support_length_estimation="FromDistributionClamped1", max_dt=0.003)
    cuts = [None] if k == 2 else [[-D.INF, -0.68, 0.65, D.INF], [-D.INF, -0.66, 0.68, D.INF], [-D.INF, -0.70, 0.62, D.INF]]
    return Group(lib, scn, P, k, 3, cuts)


@pytest.fixture(scope="module", params=["A2", "A3", "B2", "B3"])
def group(request, product_lib):
    k = int(request.param[1])
    g = (_scene_a if request.param[0] == "A" else _scene_b)(product_lib, k)
    # cuts that run through the fluid: every rank owns particles; the device (slot) order is not the id order
    assert all(len(i) > 0 for i in g.ids)
    assert any(np.any(np.diff(i.astype(np.int64)) < 0) for i in g.ids), "slot order equals id order: the test would not see a mix-up"
    if request.param[0] == "B":
        assert g.f["h2"].max() > 1.5 * g.f["h2"].min()
    yield g
    g.close()


def _pack(rgb):
    rgb = rgb.astype(np.uint64)
    return rgb[:, 0] | (rgb[:, 1] << np.uint64(8)) | (rgb[:, 2] << np.uint64(16))


def _check_layer_colours(g, attr, flags, geom):
    want = _pack(g.colors(attr, flags))
    _, bands, layers = g.layers(attr, flags, *geom)
    for r, l in enumerate(layers):
        assert l is not None
        w = l[l != 0]
        ids = (w >> np.uint64(32)).astype(np.int64) - 1
        assert w.size and np.isin(ids, g.ids[r]).all(), (attr, flags, r)
        rgb = w & np.uint64(0xffffff)
        bad = (rgb != 0) & (rgb != want[ids])
        assert not bad.any(), (attr, flags, r, int(bad.sum()))
        assert (rgb == want[ids]).any()
    got = g.group_frame(attr, flags, *geom)
    exp = g.expected(attr, flags, *geom)
    assert np.array_equal(got, exp), (attr, flags, int(np.sum(np.any(got != exp, axis=2))))


@pytest.mark.parametrize("attr", render.VISUALIZED_ATTRIBUTES)
def test_colours_every_attribute(group, attr):
    """The words of every rank's layer at a supersampled frame name only ids the rank owns and carry only the numpy colour of that id
    (or 0, the stroke band); the group frame equals numpy."""
    for flags in (0, ALL_FLAGS):
        _check_layer_colours(group, attr, flags, COLOUR_VIEW)


def test_stash_distance_colours(group):
    _check_layer_colours(group, "Distance", ffi.RENDER_FROM_STASH, COLOUR_VIEW)


def _per_rank_frames(g, product_lib, attr, w, h, s, zoom, want):
    """compose on member 0, in reversed layer order, and on a fresh plain context"""
    rp, bands, layers = g.layers(attr, 0, w, h, s, zoom)
    got = g.ctxs[0].render_compose(rp, bands, layers)
    assert np.array_equal(got, want), (attr, "per rank", int(np.sum(np.any(got != want, axis=2))))
    assert np.array_equal(g.ctxs[-1].render_compose(rp, bands[::-1], layers[::-1]), want), (attr, "reversed")
    plain = ffi.Context(product_lib, 16, g.planes)
    try:
        assert np.array_equal(plain.render_compose(rp, bands, layers), want), (attr, "plain context")
    finally:
        plain.close()
    return bands, layers


@pytest.mark.parametrize("attr,w,h,s,zoom", FRAMES + [("Density", 97, 61, 4, 1.1)])
def test_frames_equal_numpy(group, product_lib, attr, w, h, s, zoom):
    want = group.expected(attr, 0, w, h, s, zoom)
    got = group.group_frame(attr, 0, w, h, s, zoom)
    assert got.shape == (h, w, 3)
    assert np.array_equal(got, want), (attr, "group", int(np.sum(np.any(got != want, axis=2))))
    assert (got == 255).all(axis=2).any() and (got != 255).any()   # background and fluid
    _per_rank_frames(group, product_lib, attr, w, h, s, zoom, want)


def test_small_zoom_out_empty_band_and_clipped_discs(group, product_lib):
    """A view so close that a rank's slab lies outside the frame: its band is empty and it passes no layer; discs of the others are
    cut by the frame's edge."""
    # scene A: the column stands at x in [-1.97, -1], y in [-0.97, -0.2] -- a wide, low window reaches its right end only;
    # scene B: blocks at |x| in [0.4, 0.95] -- a square window that ends inside them
    geom = (400, 100, 1, 0.3) if group.f["position"][:, 0].max() < -0.5 else (200, 200, 1, 0.55)
    w, h, s, zoom = geom
    want = group.expected("Velocity", 0, *geom)
    _, keys = group.frame(*geom)
    assert keys.any() and (keys[:, 0].any() or keys[:, -1].any() or keys[0].any() or keys[-1].any()), "no disc reaches the frame's edge"
    got = group.group_frame("Velocity", 0, *geom)
    assert np.array_equal(got, want)
    bands, layers = _per_rank_frames(group, product_lib, "Velocity", w, h, s, zoom, want)
    empty = [b.sx0 == b.sx1 for b in bands]
    assert any(empty) and not all(empty), [b.as_tuple() for b in bands]
    for b, l in zip(bands, layers):
        assert (l is None) == (b.sx0 == b.sx1) and (b.n_drawn == 0) == (b.sx0 == b.sx1)


# (views that hold every rank's slab: scene A stands at x in [-2, -1])
@pytest.mark.parametrize("attr,w,h,s,zoom", [("RandomColor", 320, 160, 4, 1.05), ("Velocity", 300, 200, 1, 2.05)])
def test_layers_word_for_word(group, attr, w, h, s, zoom):
    """Every rank's downloaded layer is (id + 1) << 32 | rgb built from rr.Frame.keys over its owned particles, restricted to its band,
    and nothing is covered outside the band; adjacent bands overlap and some sample is covered in both layers (painter's order across
    the cut)."""
    _, bands, layers = group.layers(attr, 0, w, h, s, zoom)
    full = []
    for r, (b, l) in enumerate(zip(bands, layers)):
        want = group.expected_layer(r, attr, 0, w, h, s, zoom)
        assert l is not None and b.n_drawn > 0
        assert np.array_equal(l, want[:, b.sx0:b.sx1]), (r, int((l != want[:, b.sx0:b.sx1]).sum()))
        assert not want[:, :b.sx0].any() and not want[:, b.sx1:].any(), (r, "covered outside the band")
        full.append(want)
    for r in range(len(bands) - 1):
        assert bands[r + 1].sx0 < bands[r].sx1, (r, bands[r].as_tuple(), bands[r + 1].as_tuple())
        if s > 1:   # (the outer discs of neighbours across a cut overlap in a lens 0.14 spacings wide: a few samples at this scale only)
            assert ((full[r] != 0) & (full[r + 1] != 0)).any(), (r, "no sample covered from both sides of the cut")
    # the maximum of the ranks' words is the word of the whole vector's winner
    _, keys = group.frame(w, h, s, zoom)
    top = np.maximum.reduce(full)
    assert np.array_equal((top >> np.uint64(32)).astype(np.uint32), keys)


# ---- against the existing renderer ---------------------------------------------------------------------------------------------
def test_upload_state_equals_sph_render(product_lib):
    """Right after the upload (no step) a 3-slab group draws what sph_render draws for a plain context holding the same particles."""
    P = default_params(merging=False, sharing=False, splitting=False, max_dt=0.004)
    scn = sc.dam_break_small(40, 32, 1.0 / 40)
    pos, mass, vel = sc.init_particles(scn)
    vel = vel.copy()
    vel[:, 0] = np.linspace(0.0, 2.0, len(mass), dtype=np.float32)
    planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    plain = ffi.Context(product_lib, len(mass) + 64, planes)
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 3)
    try:
        plain.upload(mass, pos, vel)
        for attr in ("SingleColor", "RandomColor", "ParticleSizeClass", "Velocity"):
            want = render.render(plain, P, _vis(attr), 240, 160, 2, 1.2, planes)
            assert (want != 255).any()
            assert np.array_equal(render.render_group(grp, P, _vis(attr), 240, 160, 2, 1.2, planes), want), attr
        # no layers: the frame sph_render draws for an empty context -- background and boundary only
        empty = ffi.Context(product_lib, 16, planes)
        try:
            rp = render.render_params(_vis("Velocity"), P, 240, 160, 2, 1.2, render.boundary_segments(planes))
            want = render.render(empty, P, _vis("Velocity"), 240, 160, 2, 1.2, planes)
            assert (want != 255).any() and (want == 255).all(axis=2).any()   # the boundary strokes on the background
            assert np.array_equal(grp[1].render_compose(rp, [], []), want)
            assert np.array_equal(empty.render_compose(rp, [ffi.SphRenderBand(5, 5, 0, 0)], [None]), want)
        finally:
            empty.close()
    finally:
        plain.close()
        close_all(grp)


def test_polygon_boundary_frame(product_lib):
    P = default_params(merging=False, sharing=False, splitting=False, init_boundary_handler="AnalyticUnderestimate", max_dt=0.004)
    g = Group(product_lib, sc.dam_break_small(24, 24, 1.0 / 24), P, 2, 2)
    try:
        assert isinstance(g.planes, sc.BoundaryPolygon)
        geom = (180, 120, 2, 1.1)
        want = g.expected("Density", 0, *geom)
        assert np.array_equal(g.group_frame("Density", 0, *geom), want)
        rp, bands, layers = g.layers("Density", 0, *geom)
        assert np.array_equal(g.ctxs[0].render_compose(rp, bands, layers), want)
    finally:
        g.close()


def test_render_changes_no_state(product_lib):
    """Two identical 2-slab groups; one draws every attribute through the group call and through the per-rank calls; then both step
    twice: every downloadable field and the exported lists are equal byte for byte."""
    P = default_params(merging=False, sharing=False, splitting=False, max_dt=0.004)
    scn = sc.dam_break_small(32, 32, 1.0 / 32)
    a = Group(product_lib, scn, P, 2, 2)
    b = Group(product_lib, scn, P, 2, 2)
    try:
        for attr in render.VISUALIZED_ATTRIBUTES:
            a.group_frame(attr, ALL_FLAGS, 200, 120, 2, 1.04)
            rp, bands, layers = a.layers(attr, 0, 200, 120, 2, 1.04)
            a.ctxs[0].render_compose(rp, bands, layers)
        for _ in range(2):
            ffi.group_step(a.ctxs, a.p)
            ffi.group_step(b.ctxs, b.p)
        for x, y in zip(a.ctxs, b.ctxs):
            for f in FIELDS + ["particle_id", "cell_index", "h2_next", "level_old", "lambda_sum"]:
                assert x.download(f).tobytes() == y.download(f).tobytes(), f
            (oa, ia), (ob, ib) = x.download_neighbors(), y.download_neighbors()
            assert np.array_equal(oa, ob) and np.array_equal(ia, ib)
    finally:
        a.close()
        b.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _refused(status, word, f, *a):
    with pytest.raises(ffi.SphError) as e:
        f(*a)
    assert e.value.status == status and word in str(e.value), (status, word, e.value)


def test_refusals(product_lib):
    P = default_params(merging=False, sharing=False, splitting=False, max_dt=0.004)
    P_nolevel = P.replace(level_estimation_method="None")
    scn = sc.dam_break_small(32, 32, 1.0 / 32)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    seg = render.boundary_segments(planes)
    p = P.to_ffi()
    plain = ffi.Context(product_lib, len(mass) + 64, planes)
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 2)
    rp = render.render_params(_vis("Velocity"), P, 64, 48, 1, 2.1, seg)   # (a view that holds the whole box)

    def rp_of(attr="Velocity", w=64, h=48, s=1, zoom=2.1, alpha=None, **kw):
        q = render.render_params(_vis(attr), P, w, h, s, zoom, seg, alpha)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    try:
        plain.upload(mass, pos, vel)
        # layer, pressure maximum and download on a plain context; sph_render on a slab context still refuses
        _refused(30, "not a slab context", plain.slab_render_pressure_max)
        _refused(30, "not a slab context", plain.slab_render_layer, p, rp, 0.0)
        _refused(30, "not a slab context", plain.slab_render_layer_download)
        with pytest.raises(ffi.SphError) as e:
            render.render(grp[0], P, _vis("Velocity"), 64, 64, 1)
        assert e.value.status == 30
        # interpolation
        _refused(30, "interpolated", grp[0].slab_render_layer, p, rp_of(alpha=0.5), 0.0)
        _refused(30, "interpolated", ffi.group_render, grp, p, rp_of(alpha=0.5))
        for f in (render.render_group, render.render_rank):
            with pytest.raises(ValueError, match="alpha"):
                f(grp if f is render.render_group else grp[0], P, _vis("Velocity"), 64, 48, alpha=0.5)
        # MinDistanceToNeighbor where sph_download_neighbors refuses: no step yet
        with pytest.raises(ffi.SphError) as e:
            grp[0].download_neighbors()
        assert e.value.status == 1
        _refused(1, "MinDistanceToNeighbor", grp[0].slab_render_layer, p, rp_of("MinDistanceToNeighbor"), 0.0)
        _refused(1, "MinDistanceToNeighbor", ffi.group_render, grp, p, rp_of("MinDistanceToNeighbor"))
        # a download without a layer
        _refused(1, "no layer", grp[0].slab_render_layer_download)
        ffi.group_step(grp, p)
        grp[0].download_neighbors()
        ffi.group_render(grp, p, rp_of("MinDistanceToNeighbor"))
        # ... behind a step without level estimation the ghosts' advected positions are not their owners'
        ffi.group_step(grp, P_nolevel.to_ffi())
        _refused(1, "level estimation", grp[0].slab_render_layer, P_nolevel.to_ffi(), rp_of("MinDistanceToNeighbor"), 0.0)
        ffi.group_step(grp, p)
        # S, W, H, stops, segments, zoom: as sph_render
        for q, word in ((rp_of(s=0), "supersample"), (rp_of(s=5), "supersample"), (rp_of(w=0), "pixels"), (rp_of(h=0), "pixels"),
                        (rp_of(w=8193, h=16, s=2), "samples per side"), (rp_of(n_stops=0), "stops"), (rp_of(n_stops=17), "stops"),
                        (rp_of(n_segments=33), "segments"), (rp_of(n_segments=-1), "segments"), (rp_of(zoom_out=0.0), "zoom_out"),
                        (rp_of(attribute=12), "attribute")):
            _refused(1, word, grp[0].slab_render_layer, p, q, 0.0)
            _refused(1, word, ffi.group_render, grp, p, q)
            if word not in ("stops", "attribute"):   # (compose reads the frame geometry alone)
                _refused(1, word, plain.render_compose, q, [], [])
        buf = np.empty(64 * 48 * 3 - 1, np.uint8)
        handles = (C.c_void_p * 2)(*[c.handle for c in grp])
        assert product_lib.group_render(handles, 2, C.byref(p), C.byref(rp), buf.ctypes.data, buf.nbytes) == 1
        assert "output buffer" in product_lib.last_error(grp[0].handle).decode()
        assert product_lib.render_compose(plain.handle, C.byref(rp), 0, None, None, buf.ctypes.data, buf.nbytes) == 1
        assert "output buffer" in product_lib.last_error(plain.handle).decode()
        # a layer, then a capacity one word short
        band = grp[0].slab_render_layer(p, rp, 0.0)
        n_words = 48 * (band.sx1 - band.sx0)
        assert n_words > 1
        short = np.empty(n_words - 1, np.uint64)
        assert product_lib.slab_render_layer_download(grp[0].handle, short.ctypes.data, short.size) == 1
        assert "capacity" in product_lib.last_error(grp[0].handle).decode()
        layer = grp[0].slab_render_layer_download()
        # bands that are no column range of the frame; a NULL layer for a band that is not empty
        B = ffi.SphRenderBand
        for bad in (B(3, 2, 0, 0), B(-1, 4, 0, 0), B(0, 65, 0, 0), B(65, 65, 0, 0)):
            _refused(1, "band", plain.render_compose, rp, [bad], [np.zeros((48, max(bad.sx1 - bad.sx0, 0)), np.uint64)])
        _refused(1, "NULL", plain.render_compose, rp, [band], [None])
        plain.render_compose(rp, [band, B(64, 64, 0, 0)], [layer, None])
        # the group call: no member, a member that is no slab context
        _refused(1, "n < 1", ffi.group_render, [], p, rp)
        assert product_lib.group_render(handles, 0, C.byref(p), C.byref(rp), buf.ctypes.data, buf.nbytes) == 1
        _refused(1, "no slab context", ffi.group_render, [grp[0], plain], p, rp)
        ffi.group_step(grp, p)   # the refusals left the group able to step and to draw
        ffi.group_render(grp, p, rp)
    finally:
        plain.close()
        close_all(grp)


def test_a_poisoned_slab_group_is_not_drawn(product_lib):
    """Contexts with room for their owned particles but not for a ghost layer: the step ends in SPH_ERR_CAPACITY and leaves them
    poisoned (tests/test_gpu_slab_candidates.py); the pressure maximum, the layer and the group call answer SPH_ERR_POISONED."""
    scn = sc.dam_break_small(96, 48, 1 / 48)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    P = dam_break_params(max_iters=3, level_estimation_method="EmptyAngle", maximum_surface_distance=0.2, particle_radius_fine=0.004,
                         particle_radius_base=0.02)
    p = P.to_ffi()
    cuts = D.slab_cuts(pos[:, 0], 2)
    parts = D.partition(pos[:, 0], cuts)
    rp = render.render_params(_vis("Velocity"), P, 64, 48, 1, 1.04, render.boundary_segments(planes))
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
        _refused(31, "undefined", ffi.group_render, grp, p, rp)
        for c in grp:
            _refused(31, "undefined", c.slab_render_pressure_max)
            _refused(31, "undefined", c.slab_render_layer, p, rp, 0.0)
    finally:
        close_all(grp)
