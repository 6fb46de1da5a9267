"""Probe sets (include/sph_probe.h): the SPH interpolant at points the caller chooses -- gauges -- and points that move with the fluid's
interpolated velocity -- tracers.  The terms are those of the grid sampling (sampling.py, include/sph_sample.h): 64-bit fixed-point sums
on the device, so the raw words depend on no order and not on how the library bins the points; a probe on a lattice sample's centre
gets that sample's words.

    with ProbeSet(ctx, probes.line((0.9, -0.7), (0.9, 0.3), 64)) as gauge:
        v = gauge.sample(P, ["pressure", "velocity"])          # v.values["pressure"], v.weight
        height = probes.surface_height(v.weight, gauge.points()[:, 1])

Which state: density and pressure (and the "density" volume) are a step's outputs -- sample right behind the step, before its
adaptivity; velocity under volume="rest" is valid at any time, which is what `advect` defaults to.

Slab contexts (include/sph_slab_probe.h): every rank holds a replica of the set -- the same points in the same order -- and
`sample_group` / `advect_group` (the group of one process) or `ProbeSet.sample_rank` / `ProbeSet.advect_rank` (one process per rank)
give the words of one context that holds the same particles, bit for bit.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import ffi
from .distributed import compose_on_root
from .sampling import expand_channels


def _probe_lib(lib):
    if any(getattr(lib, s, None) is None for s in ffi.PROBE_SYMBOLS):
        raise ffi.SphError(30, f"{lib.path.name} has no probe sets (sph_probe.h is implemented by the product library only)")
    return lib


def _points(points) -> np.ndarray:
    a = np.ascontiguousarray(np.asarray(points, np.float32))
    if a.size == 0:
        return np.zeros((0, 2), np.float32)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("points must be an array of (x, y) pairs")
    return a


@dataclass
class ProbeValues:
    """What `ProbeSet.sample` returns: `values[name]` float32[n] per channel and `weight` in the caller's point order, the exponents used,
    the counters of sph_probe_info, and with raw=True the int64 words under the same names ("weight" included)."""
    names: List[str]
    values: Dict[str, np.ndarray]
    weight: np.ndarray
    exponents: Dict[str, int]
    n_touching: int
    n_pairs: int
    n_touched_points: int
    raw: Optional[Dict[str, np.ndarray]] = None
    info: Optional["ffi.SphProbeInfo"] = field(default=None, repr=False)

    def __getitem__(self, name):
        return self.weight if name == "weight" else self.values[name]


def probe_params(channels: Sequence[str], volume="density", normalize=False, min_weight=0.5, fill=float("nan"), exponents=None) -> "ffi.SphProbeParams":
    """The sph_probe_params of a call; `channels`: names of ffi.SAMPLE_CHANNELS (already expanded)."""
    pp = ffi.SphProbeParams()
    pp.volume = ffi.SAMPLE_VOLUMES[volume] if isinstance(volume, str) else int(volume)
    pp.flags = ffi.SAMPLE_NORMALIZE if normalize else 0
    pp.min_weight, pp.fill = float(min_weight), float(fill)
    pp.n_channels = len(channels)
    if exponents is not None and len(exponents) != len(channels):
        raise ValueError("one exponent (or None) per channel")
    for k, name in enumerate(channels[: ffi.SAMPLE_MAX_CHANNELS]):
        fld, comp = ffi.SAMPLE_CHANNELS[name]
        e = None if exponents is None else exponents[k]
        pp.channels[k] = ffi.SphSampleChannel(ffi.FIELDS[fld][0], comp, ffi.SAMPLE_AUTO_EXPONENT if e is None else int(e))
    return pp


def _values_of(names, values, words, info) -> ProbeValues:
    keys = ["weight"] + list(names)
    return ProbeValues(list(names), {k: values[i + 1] for i, k in enumerate(names)}, values[0],
                       {k: int(info.exponents[i]) for i, k in enumerate(names)}, int(info.n_touching), int(info.n_pairs),
                       int(info.n_touched_points), {k: words[i] for i, k in enumerate(keys)} if words is not None else None, info)


def _advect_params(dt, volume="rest", min_weight=0.5, exponents=None) -> "ffi.SphProbeAdvectParams":
    ap = ffi.SphProbeAdvectParams()
    ap.dt, ap.min_weight = float(dt), float(min_weight)
    ap.volume = ffi.SAMPLE_VOLUMES[volume] if isinstance(volume, str) else int(volume)
    ex = (None, None) if exponents is None else exponents
    ap.exponent_x, ap.exponent_y = (ffi.SAMPLE_AUTO_EXPONENT if e is None else int(e) for e in ex)
    return ap


def _velocity_params(ap) -> "ffi.SphProbeParams":
    """The sph_probe_params a tracer step folds: the two velocity channels with ap's exponents, as sph_probe_advect builds them."""
    pp = ffi.SphProbeParams()
    pp.volume, pp.min_weight, pp.n_channels = ap.volume, ap.min_weight, 2
    vel = ffi.FIELDS["velocity"][0]
    pp.channels[0] = ffi.SphSampleChannel(vel, 0, ap.exponent_x)
    pp.channels[1] = ffi.SphSampleChannel(vel, 1, ap.exponent_y)
    return pp


class _naming_the_slab_forms:
    """A slab context refuses sample / advect (status 30): the error then names the calls that serve it, around the library's sentence."""

    def __init__(self, forms):
        self.forms = forms

    def __enter__(self):
        return self

    def __exit__(self, kind, e, tb):
        if isinstance(e, ffi.SphError) and e.status == 30 and "slab contexts" in str(e):
            raise ffi.SphError(30, f"{e.message} [on slab contexts: probes.{self.forms} (include/sph_slab_probe.h)]") from None
        return False


class ProbeSet:
    """A device-resident set of points that belongs to `ctx` (sph_probe_set).  `cell_size`: 0 lets the library choose how it bins the
    points, a positive value asks for that bin size (no result depends on it).  A context manager; `close()` frees the set, and the
    context's close frees what is left."""

    def __init__(self, ctx, points, cell_size: float = 0.0):
        self.ctx = ctx
        self.lib = _probe_lib(ctx.lib)
        self.handle = None
        self.info = None   # the sph_probe_info of the last sample / advect
        pts = _points(points)
        h = C.c_void_p()
        ctx._check(self.lib.probe_set_create(ctx.handle, pts.ctypes.data if len(pts) else None, len(pts), float(cell_size), C.byref(h)))
        self.handle = h

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.handle is not None and getattr(self.ctx, "handle", None):
            handle, self.handle = self.handle, None
            self.ctx._check(self.lib.probe_set_destroy(self.ctx.handle, handle))
        self.handle = None

    def __len__(self) -> int:
        n = C.c_uint64()
        self.ctx._check(self.lib.probe_set_size(self.ctx.handle, self.handle, C.byref(n)))
        return int(n.value)

    def upload(self, points):
        """Replace the points (their number may change)."""
        pts = _points(points)
        self.ctx._check(self.lib.probe_set_upload(self.ctx.handle, self.handle, pts.ctypes.data if len(pts) else None, len(pts)))

    def points(self) -> np.ndarray:
        """float32[n, 2]: the points as they are now, in the caller's order."""
        out = np.empty((len(self), 2), np.float32)
        self.ctx._check(self.lib.probe_set_download(self.ctx.handle, self.handle, out.ctypes.data if out.size else None, out.nbytes))
        return out

    def bins(self):
        """(cell_size, cells_x, cells_y): the bin geometry the next use works with."""
        s, cx, cy = C.c_float(), C.c_int32(), C.c_int32()
        self.ctx._check(self.lib.probe_set_bins(self.ctx.handle, self.handle, C.byref(s), C.byref(cx), C.byref(cy)))
        return float(s.value), int(cx.value), int(cy.value)

    def sample(self, P, channels: Sequence[str], volume="density", normalize=False, min_weight=0.5, fill=float("nan"), raw=False,
               exponents=None) -> ProbeValues:
        """sph_probe_sample: `channels` as sampling.sample_grid takes them ("velocity" and "level" are short forms)."""
        names = expand_channels(channels)
        pp = probe_params(names, volume, normalize, min_weight, fill, exponents)
        return self.sample_params(P, pp, names, raw)

    def sample_params(self, P, pp: "ffi.SphProbeParams", names: Sequence[str], raw=False) -> ProbeValues:
        """The same with the struct given (tests hand the library parameters `probe_params` would not build)."""
        p = P.to_ffi() if hasattr(P, "to_ffi") else P
        n = len(self)
        planes = min(max(int(pp.n_channels), 0), ffi.SAMPLE_MAX_CHANNELS) + 1 if pp is not None else 1
        values = np.zeros((planes, n), np.float32)
        words = np.zeros((planes, n), np.int64) if raw else None
        info = ffi.SphProbeInfo()
        with _naming_the_slab_forms("sample_group / ProbeSet.sample_rank"):
            self.ctx._check(self.lib.probe_sample(self.ctx.handle, C.byref(p) if p is not None else None, self.handle, C.byref(pp) if pp is not None else None,
                                                  values.ctypes.data if values.size else None, values.nbytes,
                                                  words.ctypes.data if raw and words.size else None, words.nbytes if raw else 0, C.byref(info)))
        self.info = info
        return _values_of(names, values, words if raw else None, info)

    def advect(self, P, dt: float, volume="rest", min_weight=0.5, exponents=None) -> "ffi.SphProbeInfo":
        """sph_probe_advect: one explicit Euler step of every point with the interpolated velocity; a point whose weight is below
        `min_weight` stays where it is.  -> the info struct (n_moved, n_stalled, the exponents of x and y)."""
        p = P.to_ffi() if hasattr(P, "to_ffi") else P
        ap = _advect_params(dt, volume, min_weight, exponents)
        info = ffi.SphProbeInfo()
        with _naming_the_slab_forms("advect_group / ProbeSet.advect_rank"):
            self.ctx._check(self.lib.probe_advect(self.ctx.handle, C.byref(p) if p is not None else None, self.handle, C.byref(ap), C.byref(info)))
        self.info = info
        return info

    # ---- one process per rank (include/sph_slab_probe.h): every rank calls these behind the same step, on its replica of the set ----
    def _layer(self, p, pp):
        """This rank's compact layer for pp's explicit exponents -> (indices, words, (n_touching, n_pairs))"""
        info = self.ctx.slab_probe_layer(p, self.handle, pp)
        n = int(info.n_entries)
        layer = self.ctx.slab_probe_layer_download(self.handle) if n else (None, None)
        return layer[0], layer[1], (int(info.n_touching), int(info.n_pairs))

    def sample_rank(self, P, channels: Sequence[str], volume="density", normalize=False, min_weight=0.5, fill=float("nan"), raw=False,
                    exponents=None, root: int = 0) -> Optional[ProbeValues]:
        """`sample` with ONE PROCESS PER RANK.  The ranks' verdict words are all-gathered through the launcher's process group and folded
        on every rank -- every rank takes the same exponents or raises the same refusal, naming the smallest offending global id --,
        every rank packs its compact layer and sends it to `root` (distributed.compose_on_root), `root` adds the layers on its own
        replica.  Returns the values on `root`, None elsewhere; a failure on the root is re-raised on every rank."""
        import torch.distributed as dist
        names = expand_channels(channels)
        pp = probe_params(names, volume, normalize, min_weight, fill, exponents)
        p = P.to_ffi() if hasattr(P, "to_ffi") else P
        words = [None] * dist.get_world_size()
        dist.all_gather_object(words, self.ctx.slab_probe_range(p, pp).as_tuple())
        pp = ffi.probe_fold_words(self.ctx.lib, words, pp)   # (raises the same SphError on every rank)
        idx, lay, counts = self._layer(p, pp)

        def compose(parts):
            values, raw_words, info = self.ctx.probe_compose(self.handle, pp, len(self), [None if i is None else (i, w) for i, w, _ in parts], raw=raw)
            info.n_touching, info.n_pairs = sum(c[0] for _, _, c in parts), sum(c[1] for _, _, c in parts)
            self.info = info
            return _values_of(names, values, raw_words if raw else None, info)

        return compose_on_root((idx, lay, counts), compose, "probe sample", root)

    def advect_rank(self, P, dt: float, volume="rest", min_weight=0.5, exponents=None) -> "ffi.SphProbeInfo":
        """`advect` with ONE PROCESS PER RANK: the words all-gathered and folded, every rank's 3-plane layer (weight, x, y) all-gathered,
        every rank adds all layers and moves its own replica (sph_probe_compose_advect).  The move is a per-point function of integer
        sums: afterwards every rank's set holds the same points bit for bit.  -> the info struct on every rank."""
        import torch.distributed as dist
        p = P.to_ffi() if hasattr(P, "to_ffi") else P
        ap = _advect_params(dt, volume, min_weight, exponents)
        pp = _velocity_params(ap)
        world = dist.get_world_size()
        words = [None] * world
        dist.all_gather_object(words, self.ctx.slab_probe_range(p, pp).as_tuple())
        pp = ffi.probe_fold_words(self.ctx.lib, words, pp)
        ap.exponent_x, ap.exponent_y = int(pp.channels[0].exponent), int(pp.channels[1].exponent)
        parts = [None] * world
        dist.all_gather_object(parts, self._layer(p, pp))
        info = self.ctx.probe_compose_advect(self.handle, ap, [None if i is None else (i, w) for i, w, _ in parts])
        info.n_touching, info.n_pairs = sum(c[0] for _, _, c in parts), sum(c[1] for _, _, c in parts)
        self.info = info
        return info


# ---- the slab group of ONE process (the contexts ffi.group_step steps); sets[i]: a replica on contexts[i] ----
def _group_sets(contexts, sets):
    contexts, sets = list(contexts), list(sets)
    if len(contexts) != len(sets):
        raise ValueError("one probe set per context")
    return contexts, sets, [s.handle for s in sets]


def sample_group(contexts, sets, P, channels: Sequence[str], volume="density", normalize=False, min_weight=0.5, fill=float("nan"), raw=False,
                 exponents=None) -> ProbeValues:
    """`ProbeSet.sample` for a slab group: bit for bit what one context that holds the same particles returns.  The members agree on the
    exponents and the preconditions through one set of words on the device, every member scatters the particles it owns straight into
    member 0's planes (sph_group_probe_sample); only the values cross the bus."""
    contexts, sets, handles = _group_sets(contexts, sets)
    names = expand_channels(channels)
    pp = probe_params(names, volume, normalize, min_weight, fill, exponents)
    p = P.to_ffi() if hasattr(P, "to_ffi") else P
    values, words, info = ffi.group_probe_sample(contexts, p, handles, pp, len(sets[0]) if sets else 0, raw=raw)
    for s in sets:
        s.info = info
    return _values_of(names, values, words, info)


def advect_group(contexts, sets, P, dt: float, volume="rest", min_weight=0.5, exponents=None) -> "ffi.SphProbeInfo":
    """`ProbeSet.advect` for a slab group (sph_group_probe_advect): every member's replica moves from the group's summed planes;
    afterwards all of them hold the same points."""
    contexts, sets, handles = _group_sets(contexts, sets)
    p = P.to_ffi() if hasattr(P, "to_ffi") else P
    info = ffi.group_probe_advect(contexts, p, handles, _advect_params(dt, volume, min_weight, exponents))
    for s in sets:
        s.info = info
    return info


def line(p0, p1, count: int) -> np.ndarray:
    """float32[count, 2]: p0 + (k / (count - 1)) * (p1 - p0), every operation in float32; p0 alone for count == 1."""
    if count < 1:
        raise ValueError("a line has at least one point")
    a, b = np.asarray(p0, np.float32), np.asarray(p1, np.float32)
    if count == 1:
        return a.reshape(1, 2).copy()
    t = (np.arange(count, dtype=np.float32) / np.float32(count - 1)).astype(np.float32)
    return (a[None, :] + t[:, None] * (b - a)[None, :]).astype(np.float32)


def surface_height(weight, ys, threshold: float = 0.5) -> float:
    """The water height a vertical line of probes reads (host side): `weight` at the ascending heights `ys` -> the linearly interpolated y
    of the HIGHEST crossing of `threshold` going up the line (wet below, dry above).  NaN when the line is dry, ys[-1] when the line is
    wet up to its top."""
    w, y = np.asarray(weight, np.float64), np.asarray(ys, np.float64)
    if w.shape != y.shape or w.ndim != 1 or len(w) == 0:
        raise ValueError("one weight per height")
    wet = w >= threshold
    if not wet.any():
        return float("nan")
    k = int(np.flatnonzero(wet)[-1])   # the highest wet probe: the line is dry from k + 1 on
    if k == len(w) - 1:
        return float(y[-1])
    return float(y[k] + (w[k] - threshold) / (w[k] - w[k + 1]) * (y[k + 1] - y[k]))


@dataclass
class ProbeSpec:
    """A gauge file: the points in file order (`points:` first, then every line's), a label per point ("3", or "<name>[k]" on a named
    line), the fields and the volume."""
    points: np.ndarray
    labels: List[str]
    fields: List[str]
    volume: str = "density"


def load_spec(path) -> ProbeSpec:
    """YAML: `points: [[x, y], ...]`, `lines: [{from: [x, y], to: [x, y], count: n, name: s}]`, `fields: [...]` (default pressure,
    density, velocity), `volume: density | rest`."""
    import yaml
    with open(path) as fh:
        doc = yaml.safe_load(fh) or {}
    unknown = set(doc) - {"points", "lines", "fields", "volume"}
    if unknown:
        raise ValueError(f"{path}: unknown keys {sorted(unknown)}")
    pts, labels = [], []
    for xy in doc.get("points") or []:
        labels.append(str(len(pts)))
        pts.append(np.asarray(xy, np.float32).reshape(2))
    for ln in doc.get("lines") or []:
        seg = line(ln["from"], ln["to"], int(ln["count"]))
        for k, xy in enumerate(seg):
            labels.append(f"{ln['name']}[{k}]" if ln.get("name") else str(len(pts)))
            pts.append(xy)
    fields = [str(f) for f in (doc.get("fields") or ["pressure", "density", "velocity"])]
    expand_channels(fields)   # (an unknown name stops here)
    volume = str(doc.get("volume", "density"))
    if volume not in ffi.SAMPLE_VOLUMES:
        raise ValueError(f"{path}: volume {volume!r} (known: {sorted(ffi.SAMPLE_VOLUMES)})")
    return ProbeSpec(np.stack(pts).astype(np.float32) if pts else np.zeros((0, 2), np.float32), labels, fields, volume)


def csv_columns(spec: ProbeSpec) -> List[str]:
    """step, time, dt, then `<label>:<plane>` for every point and plane, the weight first."""
    planes = ["weight"] + expand_channels(spec.fields)
    return ["step", "time", "dt"] + [f"{lab}:{pl}" for lab in spec.labels for pl in planes]


def csv_row(step: int, time: float, dt: float, spec: ProbeSpec, v: ProbeValues) -> list:
    planes = ["weight"] + list(v.names)
    return [step, repr(float(time)), repr(float(dt))] + [repr(float(v[pl][k])) for k in range(len(spec.labels)) for pl in planes]
