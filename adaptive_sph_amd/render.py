"""Frames of the particle state: the host half of the reference's image harness (platform/desktop/animation/cairo_renderer.rs,
simulation/colors.rs), around the device renderer of include/sph_render.h.

The device draws the particles and the boundary lines (sph_render.hip); this file supplies what a frame is parametrised by -- the
colour maps as numbers, VisualizationParams, the boundary segments -- and what is drawn on the downloaded frame: the legend bar
(cairo_renderer.rs:112-131: gradient, 5 px frame, tick marks).  It also writes PNG files with the standard library only (zlib +
struct).

Not drawn: text.  The legend's numbers and the recipe's `title` need a font rasteriser, which the project does not have; a recipe
that asks for them gets its image without them and one warning per process.
"""
from __future__ import annotations

import ctypes as C
import struct
import sys
import zlib
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import ffi
from .distributed import compose_on_root

f32 = np.float32

# VisualizedAttribute (simulation.rs:2804-2817): position = the enum value of include/sph_render.h
VISUALIZED_ATTRIBUTES = ["Distance", "SingleColor", "ParticleSizeClass", "Pressure", "Density", "Velocity", "RandomColor", "Aii",
                         "NeighborCount", "MinDistanceToNeighbor", "ConstantField", "SourceTerm"]
DRAW_SHAPES = ["Dot", "Circle", "FilledCircle", "FilledCircleWithBorder"]   # simulation.rs:2854-2866 (the renderer draws the last)

# colors.rs:17-84 color_map_inferno and :86-154 color_map_viridis: (fraction of [min, max], r, g, b)
INFERNO = [(0.0, 0.0014619955811715805, 0.0004659913919114934, 0.013866005775115809),
           (0.06666666666666667, 0.04691458399133113, 0.030323540520811973, 0.15016326468244964),
           (0.13333333333333333, 0.14237847430795506, 0.04624117675574093, 0.30855378680836465),
           (0.2, 0.2582339375612672, 0.038569281262784215, 0.4064850812186898),
           (0.26666666666666666, 0.366528457743285, 0.07157684449494817, 0.4319940445656597),
           (0.3333333333333333, 0.47232856222023284, 0.11054509253877559, 0.428334014815688),
           (0.4, 0.5783040710826255, 0.1480366969821801, 0.4044110859921461),
           (0.4666666666666667, 0.6826555952415246, 0.1894982847225483, 0.3607573457624624),
           (0.5333333333333333, 0.780517595641067, 0.24332476411029125, 0.29952273568573573),
           (0.6, 0.865006157141607, 0.316819514079576, 0.2260550749407627),
           (0.6666666666666666, 0.9296439014941755, 0.41147612778815296, 0.14536750158970949),
           (0.7333333333333333, 0.970919318954511, 0.5228513513717987, 0.05836666742473027),
           (0.8, 0.987622172670732, 0.6453178289458518, 0.039886017500422775),
           (0.8666666666666667, 0.9788062634501479, 0.7745421938654863, 0.1760361942373471),
           (0.9333333333333333, 0.950018012245954, 0.9034074125145412, 0.3802723264284489),
           (1.0, 0.9883620799212208, 0.9983616470620554, 0.6449240982803861)]
VIRIDIS = [(0.0, 0.2670039853213788, 0.0048725657145795975, 0.32941506855247793),
           (0.06666666666666667, 0.28265591676374746, 0.10019440706631136, 0.42215967285462885),
           (0.13333333333333333, 0.27713381181214125, 0.18522747944269774, 0.4898983578428951),
           (0.2, 0.25393482507335086, 0.26525311670734747, 0.529983099667603),
           (0.26666666666666666, 0.22198891605799553, 0.33915975136273824, 0.5487520417750932),
           (0.3333333333333333, 0.19063051802725675, 0.4070603881536437, 0.5560891205440711),
           (0.4, 0.1636245598287687, 0.47113199888460483, 0.5581480982786068),
           (0.4666666666666667, 0.13914656229528236, 0.5338106140906136, 0.555298125858835),
           (0.5333333333333333, 0.12056429075653713, 0.5964211612480832, 0.5436109978665574),
           (0.6, 0.1346914034616326, 0.6586347623899736, 0.5176490803131216),
           (0.6666666666666666, 0.2080291781284243, 0.7186993731402823, 0.47287333975819085),
           (0.7333333333333333, 0.32779655496333804, 0.7739788075712202, 0.40663965647349865),
           (0.8, 0.47750397699915853, 0.8214424087022711, 0.3181950138984179),
           (0.8666666666666667, 0.6472561782044223, 0.8583980753432965, 0.2098615478515251),
           (0.9333333333333333, 0.8249409891695173, 0.8847181273467387, 0.10621658195896774),
           (1.0, 0.9932481489335602, 0.9061547634208059, 0.14393594366968385)]


class ColorMap:
    """ColorMap (color_map.rs:7-30) in f32: stops sorted by value at construction, `get` clamps at both ends and interpolates
    linearly, c0 + t * (c1 - c0).  A NaN value takes the first stop's colour (the reference panics there)."""

    def __init__(self, insertions: Sequence[Tuple[float, Sequence[float]]]):
        st = [(f32(v), tuple(f32(x) for x in c)) for v, c in insertions]
        st.sort(key=lambda s: float(s[0]))     # slice::sort_by: stable
        self.insertions = st

    def get(self, x) -> Tuple[np.float32, np.float32, np.float32]:
        x = f32(x)
        st = self.insertions
        if np.isnan(x) or x <= st[0][0]:
            return st[0][1]
        if x >= st[-1][0]:
            return st[-1][1]
        for (v0, c0), (v1, c1) in zip(st[:-1], st[1:]):
            if v0 <= x <= v1:
                t = f32(f32(x - v0) / f32(v1 - v0))
                return tuple(f32(a + f32(t * f32(b - a))) for a, b in zip(c0, c1))
        return st[0][1]

    def color_stops(self):
        return self.insertions


def _from_table(table, lo, hi) -> ColorMap:
    lo, hi = f32(lo), f32(hi)
    return ColorMap([(f32(lo + f32(f32(hi - lo) * f32(fr))), (r, g, b)) for fr, r, g, b in table])


def color_map_inferno(lo, hi) -> ColorMap:
    return _from_table(INFERNO, lo, hi)


def color_map_viridis(lo, hi) -> ColorMap:
    return _from_table(VIRIDIS, lo, hi)


def color_map_for_pressure(max_pressure) -> ColorMap:
    """get_color_map_for_pressure (colors.rs:289-298)."""
    return ColorMap([(0.0, (1.0, 1.0, 1.0)), (max_pressure, (1.0, 0.0, 0.0))])


def get_color_map(attr: str, simulation_params) -> Optional[ColorMap]:
    """get_color_map (colors.rs:300-384): the fixed map of an attribute, None for Pressure / RandomColor / SingleColor /
    ParticleSizeClass."""
    if attr == "SourceTerm":
        return color_map_viridis(-6000.0, 6000.0)
    if attr == "Aii":
        return ColorMap([(-1.0, (1, 0, 0)), (0.0, (1, 1, 1)), (50.0, (0, 0, 1))])
    if attr == "Distance":
        return color_map_inferno(-f32(simulation_params.maximum_surface_distance), 0.0)
    if attr == "Velocity":
        return color_map_viridis(0.0, 4.0)
    if attr == "Density":
        return ColorMap([(0.9, (0, 0, 1)), (1.0, (1, 1, 1)), (1.01, (1, 0, 0))])
    if attr == "NeighborCount":
        return ColorMap([(-4.0, (0, 0, 1)), (-2.0, (0, 1, 1)), (0.0, (0, 1, 0)), (2.0, (1, 1, 0)), (4.0, (1, 0, 0))])
    if attr == "ConstantField":
        diff = f32(1.05)
        return ColorMap([(f32(2.0) - diff, (0, 0, 1)), (1.0, (1, 1, 1)), (diff, (1, 0, 0))])
    if attr == "MinDistanceToNeighbor":
        return ColorMap([(0.0, (1, 0, 0)), (0.1, (1, 1, 0)), (0.3, (0, 1, 0)), (1.0, (0, 0, 1)), (1.2, (1, 0, 1))])
    if attr in ("Pressure", "RandomColor", "SingleColor", "ParticleSizeClass"):
        return None
    raise ValueError(f"unknown variant `{attr}`, expected one of {VISUALIZED_ATTRIBUTES}")


@dataclass(frozen=True)
class VisualizationParams:
    """VisualizationParams (simulation.rs:2875-2888); serde's defaults for the optional keys, unknown keys ignored."""
    visualized_attribute: str
    draw_shape: str = "FilledCircleWithBorder"
    draw_support_radius: bool = False
    show_flag_is_fluid_surface: bool = False
    show_flag_neighborhood_reduced: bool = False
    take_data_from_stash: bool = False

    @classmethod
    def from_mapping(cls, m) -> "VisualizationParams":
        if not isinstance(m, dict):
            raise TypeError("visualization_params: expected a mapping")
        if "visualized_attribute" not in m:
            raise KeyError("missing field `visualized_attribute`")
        attr = str(m["visualized_attribute"])
        if attr not in VISUALIZED_ATTRIBUTES:
            raise ValueError(f"unknown variant `{attr}`, expected one of {VISUALIZED_ATTRIBUTES}")
        shape = str(m.get("draw_shape", "FilledCircleWithBorder"))
        if shape not in DRAW_SHAPES:
            raise ValueError(f"unknown variant `{shape}`, expected one of {DRAW_SHAPES}")
        kw = {}
        for k in ("draw_support_radius", "show_flag_is_fluid_surface", "show_flag_neighborhood_reduced", "take_data_from_stash"):
            v = m.get(k, False)
            if not isinstance(v, bool):
                raise TypeError(f"invalid type for {k}: expected a boolean, got {v!r}")
            kw[k] = v
        return cls(attr, shape, **kw)


def boundary_segments(planes) -> List[Tuple[float, float, float, float]]:
    """The lines render2d strokes (cairo_renderer.rs:63-86): an SdfPlane as get_two_points_with_distance(5) (sdf_plane.rs:22-28),
    an Sdf2D polygon as draw_lines (sdf2d.rs:167-178: every edge, the last one closing the polygon).  `planes`: what
    scene.boundary_planes returns (a list of (dir_x, dir_y, delta) or a BoundaryPolygon)."""
    pts = getattr(planes, "points", None)
    if pts is not None:
        n = len(pts)
        return [(float(f32(pts[i][0])), float(f32(pts[i][1])), float(f32(pts[(i + 1) % n][0])), float(f32(pts[(i + 1) % n][1])))
                for i in range(n)]
    out = []
    half = f32(5.0)
    for dx, dy, delta in planes:
        dx, dy, delta = f32(dx), f32(dy), f32(delta)
        lx, ly = -dy, dx                       # line_dir = (-dir.y, dir.x)
        ox, oy = f32(lx * half) / f32(2.0), f32(ly * half) / f32(2.0)
        px, py = f32(dx * delta), f32(dy * delta)
        out.append((float(f32(px + ox)), float(f32(py + oy)), float(f32(px - ox)), float(f32(py - oy))))
    return out


LINE_WIDTH = 5.0 / 1000.0   # cairo_renderer.rs:73, 80


def render_params(vis: VisualizationParams, simulation_params, width: int, height: int, supersample: int = 1, zoom_out: float = 1.04,
                  segments=(), alpha: Optional[float] = None, line_width: float = LINE_WIDTH) -> ffi.SphRenderParams:
    """VisualizationParams + frame geometry -> sph_render_params.  The colour map of the attribute travels as numbers."""
    rp = ffi.SphRenderParams()
    rp.width, rp.height, rp.supersample = int(width), int(height), int(supersample)
    rp.zoom_out = float(zoom_out)
    rp.attribute = VISUALIZED_ATTRIBUTES.index(vis.visualized_attribute)
    flags = 0
    if vis.show_flag_is_fluid_surface:
        flags |= ffi.RENDER_SHOW_SURFACE
    if vis.show_flag_neighborhood_reduced:
        flags |= ffi.RENDER_SHOW_NEIGHBORHOOD_REDUCED
    if vis.take_data_from_stash:
        flags |= ffi.RENDER_FROM_STASH
    if alpha is not None:
        flags |= ffi.RENDER_INTERPOLATE
        rp.alpha = float(alpha)
    rp.flags = flags
    cmap = get_color_map(vis.visualized_attribute, simulation_params)
    if cmap is not None:
        stops = cmap.color_stops()
        if len(stops) > ffi.RENDER_MAX_STOPS:
            raise ValueError(f"a colour map of {len(stops)} stops (the renderer takes {ffi.RENDER_MAX_STOPS})")
        rp.n_stops = len(stops)
        for k, (v, c) in enumerate(stops):
            rp.stops[k][0], rp.stops[k][1], rp.stops[k][2], rp.stops[k][3] = float(v), float(c[0]), float(c[1]), float(c[2])
    seg = np.ascontiguousarray(np.asarray(segments, np.float32).reshape(-1, 4))
    rp.n_segments = int(seg.shape[0])
    rp._segments_keepalive = seg                   # the pointer below must outlive the call
    rp.segments = seg.ctypes.data_as(C.POINTER(C.c_float)) if seg.size else C.POINTER(C.c_float)()
    rp.line_width = float(line_width)
    return rp


def render(ctx: ffi.Context, simulation_params, vis: VisualizationParams, width: int = 2000, height: int = 2000, supersample: int = 1,
           zoom_out: float = 1.04, planes=(), alpha: Optional[float] = None) -> np.ndarray:
    """The frame of the context's current state as uint8[height, width, 3] (top row first), drawn on the device."""
    p = simulation_params.to_ffi() if hasattr(simulation_params, "to_ffi") else simulation_params
    rp = render_params(vis, simulation_params, width, height, supersample, zoom_out, boundary_segments(planes), alpha)
    return ctx.render_frame(p, rp)


def render_colors(ctx: ffi.Context, simulation_params, vis: VisualizationParams) -> np.ndarray:
    """The colour pass alone: uint8[n, 3] in reference order (e.g. a colour column for a VTK file)."""
    p = simulation_params.to_ffi() if hasattr(simulation_params, "to_ffi") else simulation_params
    return ctx.render_colors(p, render_params(vis, simulation_params, 1, 1))


# ---- frames from slab contexts (include/sph_slab_render.h) ------------------------------------------------------------------
def _slab_frame_params(name, simulation_params, vis, width, height, supersample, zoom_out, planes, alpha):
    if alpha is not None:
        raise ValueError(f"{name}: interpolated frames (alpha) are not drawn from slab contexts -- a particle may have changed rank since the snapshot")
    p = simulation_params.to_ffi() if hasattr(simulation_params, "to_ffi") else simulation_params
    return p, render_params(vis, simulation_params, width, height, supersample, zoom_out, boundary_segments(planes))


def render_group(contexts, simulation_params, vis: VisualizationParams, width: int = 2000, height: int = 2000, supersample: int = 1,
                 zoom_out: float = 1.04, planes=(), alpha: Optional[float] = None) -> np.ndarray:
    """The frame of a slab group of ONE process (the contexts ffi.group_step steps) as uint8[height, width, 3]: byte for byte what
    `render` draws for one context that holds the same particles.  Every member draws the particles it owns into a layer of
    (id + 1) << 32 | rgb words, member 0 takes the per-sample maximum on the device (sph_group_render); only the frame crosses the bus."""
    p, rp = _slab_frame_params("render_group", simulation_params, vis, width, height, supersample, zoom_out, planes, alpha)
    return ffi.group_render(contexts, p, rp)


def render_rank(ctx: ffi.Context, simulation_params, vis: VisualizationParams, width: int = 2000, height: int = 2000, supersample: int = 1,
                zoom_out: float = 1.04, planes=(), alpha: Optional[float] = None, root: int = 0) -> Optional[np.ndarray]:
    """The same frame with ONE PROCESS PER RANK: every rank calls this behind the same step.  The pressure maximum is all-gathered,
    every rank draws its layer and sends `root` its (band, layer) through the launcher's process group (torch.distributed
    gather_object, as distributed.rank_single_step_adaptivity_on_slabs sends its rows), `root` composes them on its own context.
    Returns the frame on `root`, None elsewhere; a failure on the root is re-raised on every rank."""
    import torch.distributed as dist
    p, rp = _slab_frame_params("render_rank", simulation_params, vis, width, height, supersample, zoom_out, planes, alpha)
    pmax = 0.0
    if vis.visualized_attribute == "Pressure":
        vals = [None] * dist.get_world_size()
        dist.all_gather_object(vals, ctx.slab_render_pressure_max())
        pmax = max(vals)   # (an f32 maximum: the same on every rank whatever the order)
    band = ctx.slab_render_layer(p, rp, pmax)
    layer = ctx.slab_render_layer_download() if band.sx1 > band.sx0 else None

    def compose(parts):
        bands = [ffi.SphRenderBand(b[0], b[1], b[2], 0) for b, _ in parts]
        return ctx.render_compose(rp, bands, [l for _, l in parts])

    return compose_on_root((band.as_tuple(), layer), compose, "render", root)


def _u8(c) -> np.ndarray:
    return np.clip(np.floor(np.asarray(c, np.float32) * f32(255.0) + f32(0.5)), 0, 255).astype(np.uint8)


def draw_legend(img: np.ndarray, color_map: ColorMap, text_right: bool = False, only_min_max: bool = False) -> np.ndarray:
    """The legend bar of cairo_renderer.rs:112-131 drawn into `img` (uint8[H, W, 3], modified in place and returned): the
    colour map's gradient in a box at x in [0.83 W, 0.90 W], y in [0.2 H, 0.5 H] (minimum at the bottom), a 5 px black frame and
    a tick mark of 0.01 W at every stop (or at the two ends with only_min_max), on the side the numbers would be.  Pixels are
    painted where their centre lies inside a shape; the numbers themselves are not drawn (no font rasteriser)."""
    H, W = img.shape[:2]
    x0, bw = W * 0.83, W * 0.07
    y_lo, bh = H * 0.5, H * 0.3                  # cairo's flipped frame: legend_min.y from the bottom
    top, bottom = H - (y_lo + bh), H - y_lo
    stops = color_map.color_stops()
    vmin, vmax = float(stops[0][0]), float(stops[-1][0])
    xc = np.arange(W) + 0.5
    yc = np.arange(H) + 0.5
    inside_x = (xc >= x0) & (xc < x0 + bw)
    rows = np.nonzero((yc >= top) & (yc < bottom))[0]
    for r in rows:
        frac = (bottom - yc[r]) / bh
        v = vmin + frac * (vmax - vmin)
        img[r, inside_x] = _u8(color_map.get(v))
    lw = 2.5
    X, Y = np.meshgrid(xc, yc)
    outer = (X >= x0 - lw) & (X < x0 + bw + lw) & (Y >= top - lw) & (Y < bottom + lw)
    inner = (X >= x0 + lw) & (X < x0 + bw - lw) & (Y >= top + lw) & (Y < bottom - lw)
    img[outer & ~inner] = 0
    ind = W * 0.01
    ticks = [vmin, vmax] if only_min_max else [float(v) for v, _ in stops]
    for v in ticks:
        interp = (v - vmin) / (vmax - vmin) if vmax != vmin else 0.0
        ycen = H - (y_lo + interp * bh)
        xa, xb = (x0 + bw, x0 + bw + ind) if text_right else (x0 - ind, x0)
        img[(X >= xa) & (X < xb) & (Y >= ycen - lw) & (Y < ycen + lw)] = 0
    return img


_WARNED = set()


def warn_once(key: str, text: str) -> None:
    if key not in _WARNED:
        _WARNED.add(key)
        print(f"warning: {text}", file=sys.stderr)


# ---- PNG (RFC 2083) with the standard library ------------------------------------------------------------------------------
def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def encode_png(img: np.ndarray) -> bytes:
    """uint8[H, W, 3] -> the bytes of an 8-bit RGB PNG (filter type 0 on every row)."""
    img = np.ascontiguousarray(img, np.uint8)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("expected an RGB image of shape (H, W, 3)")
    H, W = img.shape[:2]
    raw = np.concatenate([np.zeros((H, 1), np.uint8), img.reshape(H, W * 3)], axis=1).tobytes()
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(raw, 6)) + _chunk(b"IEND", b""))


def write_png(path, img: np.ndarray) -> None:
    with open(path, "wb") as fh:
        fh.write(encode_png(img))


def decode_png(data: bytes) -> np.ndarray:
    """The inverse of encode_png for 8-bit RGB files without interlacing (filter types 0-4); checks every chunk's CRC."""
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG file")
    pos, idat, hdr = 8, b"", None
    while pos < len(data):
        (length,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        if zlib.crc32(tag + body) & 0xffffffff != crc:
            raise ValueError(f"CRC mismatch in chunk {tag!r}")
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat += body
        elif tag == b"IEND":
            break
        pos += 12 + length
    W, H, depth, ctype, _, _, interlace = hdr
    if depth != 8 or ctype != 2 or interlace != 0:
        raise ValueError("only 8-bit RGB, non-interlaced")
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + W * 3)
    out = np.zeros((H, W * 3), np.int32)
    prev = np.zeros(W * 3, np.int32)
    for r in range(H):
        ft, line = raw[r, 0], raw[r, 1:].astype(np.int32)
        if ft == 0:
            out[r] = prev = line
            continue
        cur = np.zeros(W * 3, np.int32)
        for x in range(W * 3):
            a = cur[x - 3] if x >= 3 else 0
            b = prev[x]
            c = prev[x - 3] if x >= 3 else 0
            if ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) // 2
            else:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            cur[x] = (line[x] + pred) & 0xff
        out[r] = cur
        prev = cur
    return out.reshape(H, W, 3).astype(np.uint8)
