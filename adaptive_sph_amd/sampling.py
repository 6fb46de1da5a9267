"""SPH fields on a regular grid, sampled on the device (include/sph_sample.h): the parameters of `Context.sample_grid`, named planes,
and `resolve`, the host twin of the device's last kernel; `sample_group` and `sample_rank` give the same planes from slab contexts
(include/sph_slab_sample.h).

The device accumulates every sum as a 64-bit fixed-point integer, so the RAW planes do not depend on any order and the raw planes of
disjoint particle sets add exactly: a host that holds the layers of several contexts adds them and resolves the sum with `resolve`.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import ffi
from .distributed import compose_on_root

# the channel names `sample_grid` takes; "velocity" is short for its two components, "level" for "level_estimation"
CHANNEL_ALIASES = {"velocity": ("velocity_x", "velocity_y"), "level": ("level_estimation",)}


@dataclass(frozen=True)
class GridSpec:
    """nx x ny samples; sample (sx, sy) sits at origin + (s + 0.5) * spacing, row 0 = the LOWEST y."""
    nx: int
    ny: int
    origin: Tuple[float, float]
    spacing: float

    @classmethod
    def covering(cls, boundary, spacing: float, margin: float = 0.0) -> "GridSpec":
        """The grid over a scene's boundary box (scene.SceneBoundary: centred on the origin), `margin` scene units wider on every side."""
        w, h = float(boundary.width) + 2.0 * margin, float(boundary.height) + 2.0 * margin
        nx, ny = max(1, math.ceil(w / spacing - 1e-9)), max(1, math.ceil(h / spacing - 1e-9))
        return cls(nx, ny, (-0.5 * w, -0.5 * h), float(spacing))

    def centers(self):
        """(X[nx], Y[ny]) float32, the arithmetic of sph_sample.h."""
        f = np.float32
        X = f(self.origin[0]) + (np.arange(self.nx, dtype=np.float32) + f(0.5)) * f(self.spacing)
        Y = f(self.origin[1]) + (np.arange(self.ny, dtype=np.float32) + f(0.5)) * f(self.spacing)
        return X, Y


def expand_channels(channels: Sequence[str]):
    """"velocity" -> its two components, "level" -> "level_estimation"; the order is kept."""
    out = []
    for c in channels:
        for name in CHANNEL_ALIASES.get(c, (c,)):
            if name not in ffi.SAMPLE_CHANNELS:
                raise ValueError(f"unknown channel {c!r} (known: {sorted(ffi.SAMPLE_CHANNELS) + sorted(CHANNEL_ALIASES)})")
            out.append(name)
    return out


def sample_params(grid: GridSpec, channels: Sequence[str], volume="density", normalize=False, min_weight=0.5, fill=float("nan"),
                  exponents=None) -> "ffi.SphSampleParams":
    """The sph_sample_params of a call.  `channels`: names of ffi.SAMPLE_CHANNELS (already expanded), at most as many as the struct
    holds -- the library refuses the rest; `exponents`: None (all automatic) or one int / None per channel."""
    sp = ffi.SphSampleParams()
    sp.nx, sp.ny = int(grid.nx), int(grid.ny)
    sp.origin_x, sp.origin_y, sp.spacing = float(grid.origin[0]), float(grid.origin[1]), float(grid.spacing)
    sp.volume = ffi.SAMPLE_VOLUMES[volume] if isinstance(volume, str) else int(volume)
    sp.flags = ffi.SAMPLE_NORMALIZE if normalize else 0
    sp.min_weight, sp.fill = float(min_weight), float(fill)
    sp.n_channels = len(channels)
    if exponents is not None and len(exponents) != len(channels):
        raise ValueError("one exponent (or None) per channel")
    for k, name in enumerate(channels[: ffi.SAMPLE_MAX_CHANNELS]):
        field, comp = ffi.SAMPLE_CHANNELS[name]
        e = None if exponents is None else exponents[k]
        sp.channels[k] = ffi.SphSampleChannel(ffi.FIELDS[field][0], comp, ffi.SAMPLE_AUTO_EXPONENT if e is None else int(e))
    return sp


@dataclass
class SampledPlanes:
    """What `sample_grid` returns: `planes["weight"]` and one float32[ny, nx] per channel (row 0 = the lowest y), the exponents used,
    the counts of sph_sample_info (particles that touch a sample, the largest footprint, the (particle, sample) pairs), and with
    raw=True the int64 planes under the same names."""
    grid: GridSpec
    planes: Dict[str, np.ndarray]
    exponents: Dict[str, int]
    n_touching: int
    max_footprint: int
    n_pairs: int
    raw: Optional[Dict[str, np.ndarray]] = None

    def __getitem__(self, name):
        return self.planes[name]


def sample_grid(ctx, P, grid: GridSpec, channels: Sequence[str], volume="density", normalize=False, min_weight=0.5, fill=float("nan"),
                exponents=None, raw=False, host=None) -> SampledPlanes:
    """Sample `channels` of the context's state on `grid` (sph_sample_grid).  `P`: SimulationParams or an ffi.SphParams; `host`:
    ffi.HostBuffers to receive the planes in (views, overwritten by the next call) instead of fresh arrays."""
    names = expand_channels(channels)
    sp = sample_params(grid, names, volume, normalize, min_weight, fill, exponents)
    p = P.to_ffi() if hasattr(P, "to_ffi") else P
    values, planes, info = ctx.sample_grid(p, sp, raw=raw, host=host)
    return _planes_of(grid, names, values, planes, info.exponents, (info.n_touching, info.max_footprint, info.n_pairs), raw)


def resolve(raw: np.ndarray, exponents: Sequence[int], normalize=False, min_weight=0.5, fill=float("nan")) -> np.ndarray:
    """The host twin of k_sample_resolve: raw int64[C+1, ny, nx] (plane 0 = the weight's sums) and the C exponents -> float32 planes,
    bit for bit what the device returns for the same raw planes."""
    raw = np.asarray(raw, np.int64)
    if raw.ndim != 3 or raw.shape[0] != len(exponents) + 1:
        raise ValueError("raw must be int64[C+1, ny, nx] with one exponent per channel")
    out = np.empty(raw.shape, np.float32)
    weight = (raw[0].astype(np.float64) * 2.0 ** -32).astype(np.float32)
    out[0] = weight
    keep = weight >= np.float32(min_weight)
    for c, e in enumerate(exponents):
        v = (raw[c + 1].astype(np.float64) * 2.0 ** (int(e) - 32)).astype(np.float32)
        if normalize:
            with np.errstate(divide="ignore", invalid="ignore"):
                v = np.where(keep, v / weight, np.float32(fill)).astype(np.float32)
        out[c + 1] = v
    return out


# ---- the same planes from slab contexts (include/sph_slab_sample.h) --------------------------------------------------------------
def _planes_of(grid, names, values, planes, exponents, counts, raw) -> SampledPlanes:
    keys = ["weight"] + names
    return SampledPlanes(grid, {k: values[i] for i, k in enumerate(keys)}, {k: int(exponents[i]) for i, k in enumerate(names)},
                         int(counts[0]), int(counts[1]), int(counts[2]), {k: planes[i] for i, k in enumerate(keys)} if raw else None)


def sample_group(contexts, P, grid: GridSpec, channels: Sequence[str], volume="density", normalize=False, min_weight=0.5, fill=float("nan"),
                 exponents=None, raw=False, host=None) -> SampledPlanes:
    """The planes of a slab group of ONE process (the contexts ffi.group_step steps): bit for bit what `sample_grid` returns for one
    context that holds the same particles.  The members agree on the exponents and the preconditions through one set of words on the
    device, every member scatters the particles it owns into a layer of int64 sums, member 0 adds the layers (sph_group_sample_grid);
    only the planes cross the bus.  Keywords as `sample_grid`."""
    names = expand_channels(channels)
    sp = sample_params(grid, names, volume, normalize, min_weight, fill, exponents)
    p = P.to_ffi() if hasattr(P, "to_ffi") else P
    values, planes, info = ffi.group_sample_grid(contexts, p, sp, raw=raw, host=host)
    return _planes_of(grid, names, values, planes, info.exponents, (info.n_touching, info.max_footprint, info.n_pairs), raw)


def sample_rank(ctx, P, grid: GridSpec, channels: Sequence[str], volume="density", normalize=False, min_weight=0.5, fill=float("nan"),
                exponents=None, raw=False, host=None, root: int = 0) -> Optional[SampledPlanes]:
    """The same planes with ONE PROCESS PER RANK: every rank calls this behind the same step.  The ranks' verdict words are
    all-gathered through the launcher's process group (torch.distributed all_gather_object) and folded on every rank -- every rank
    takes the same exponents or raises the same refusal, naming the smallest offending global id --, every rank scatters its layer
    and sends `root` its (band, counts, layer) (gather_object, as render.render_rank sends its layers), `root` composes them on its own
    context.  Returns the planes on `root`, None elsewhere; a failure on the root is re-raised on every rank."""
    import torch.distributed as dist
    names = expand_channels(channels)
    sp = sample_params(grid, names, volume, normalize, min_weight, fill, exponents)
    p = P.to_ffi() if hasattr(P, "to_ffi") else P
    words = [None] * dist.get_world_size()
    dist.all_gather_object(words, ctx.slab_sample_range(p, sp).as_tuple())
    sp = ffi.sample_fold_words(ctx.lib, words, sp)   # (raises the same SphError on every rank)
    band, info = ctx.slab_sample_layer(p, sp)
    layer = ctx.slab_sample_layer_download() if band.sx1 > band.sx0 else None

    def compose(parts):
        bands = [ffi.SphSampleBand(b[0], b[1], b[2], 0) for b, _, _ in parts]
        values, planes = ctx.sample_compose(sp, bands, [l for _, _, l in parts], raw=raw, host=host)
        counts = (sum(c[0] for _, c, _ in parts), max(c[1] for _, c, _ in parts), sum(c[2] for _, c, _ in parts))
        return _planes_of(grid, names, values, planes, [sp.channels[k].exponent for k in range(len(names))], counts, raw)

    mine = (band.as_tuple(), (int(info.n_touching), int(info.max_footprint), int(info.n_pairs)), layer)
    return compose_on_root(mine, compose, "sample", root)
