"""TEST INFRASTRUCTURE: a numpy restatement of the device renderer (include/sph_render.h, adaptive_sph_amd/csrc/sph_render.hip).

Every operation is one f32 operation in the order the header states, so the colours and the frames come out byte for byte as the
device draws them.  Inputs are host arrays in reference order (what sph_download / sph_download_neighbors return).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

f32 = np.float32
MASK64 = (1 << 64) - 1
FRAC_1_PI = f32(0.318309873342514038086)
ETA = f32(1.9)


# ---- SipHash-c-d (Aumasson & Bernstein), 64-bit output ---------------------------------------------------------------------
def _rotl(x: int, b: int) -> int:
    return ((x << b) | (x >> (64 - b))) & MASK64


def siphash(message: bytes, k0: int = 0, k1: int = 0, c: int = 2, d: int = 4) -> int:
    v0, v1 = k0 ^ 0x736f6d6570736575, k1 ^ 0x646f72616e646f6d
    v2, v3 = k0 ^ 0x6c7967656e657261, k1 ^ 0x7465646279746573

    def rounds(k):
        nonlocal v0, v1, v2, v3
        for _ in range(k):
            v0 = (v0 + v1) & MASK64; v1 = _rotl(v1, 13); v1 ^= v0; v0 = _rotl(v0, 32)
            v2 = (v2 + v3) & MASK64; v3 = _rotl(v3, 16); v3 ^= v2
            v0 = (v0 + v3) & MASK64; v3 = _rotl(v3, 21); v3 ^= v0
            v2 = (v2 + v1) & MASK64; v1 = _rotl(v1, 17); v1 ^= v2; v2 = _rotl(v2, 32)

    n = len(message)
    tail = n - n % 8
    for off in range(0, tail, 8):
        m = int.from_bytes(message[off:off + 8], "little")
        v3 ^= m
        rounds(c)
        v0 ^= m
    b = ((n & 0xff) << 56) | int.from_bytes(message[tail:], "little")
    v3 ^= b
    rounds(c)
    v0 ^= b
    v2 ^= 0xff
    rounds(d)
    return v0 ^ v1 ^ v2 ^ v3


def rust_default_hash_usize(i: int) -> int:
    """Rust's DefaultHasher::new() (SipHash-1-3, keys 0) after `(i as usize).hash(&mut s)`: the 8 little-endian bytes."""
    return siphash(int(i).to_bytes(8, "little"), 0, 0, 1, 3)


# ---- colour pass ----------------------------------------------------------------------------------------------------------
def _u8(c) -> np.ndarray:
    t = np.floor(np.asarray(c, f32) * f32(255.0) + f32(0.5))
    return np.clip(t, f32(0), f32(255)).astype(np.uint8)


def cmap_get(stops: Sequence, x) -> np.ndarray:
    """ColorMap::get over an array: stops = [(value, r, g, b), ...] ascending -> uint8[n, 3]."""
    x = np.asarray(x, f32)
    v = [f32(s[0]) for s in stops]
    c = [[f32(s[1]), f32(s[2]), f32(s[3])] for s in stops]
    out = np.zeros((x.shape[0], 3), f32)
    last = len(stops) - 1
    first = np.isnan(x) | (x <= v[0])
    done = first.copy()
    out[first] = c[0]
    hi = ~done & (x >= v[last])
    out[hi] = c[last]
    done |= hi
    for k in range(last):
        m = ~done & (x >= v[k]) & (x <= v[k + 1])
        if m.any():
            t = (x[m] - v[k]) / (v[k + 1] - v[k])
            for ch in range(3):
                out[m, ch] = c[k][ch] + t * (c[k + 1][ch] - c[k][ch])
        done |= m
    out[~done] = c[0]
    return _u8(out)


def min_distance_to_neighbor(position, h, offsets, indices) -> np.ndarray:
    """min over j in list(i), j != i, of sqrt(dx*dx + dy*dy) / h_i, chained with 2 (colors.rs:460-472)."""
    n = position.shape[0]
    rows = np.repeat(np.arange(n), np.diff(offsets.astype(np.int64)))
    cols = indices.astype(np.int64)
    keep = rows != cols
    rows, cols = rows[keep], cols[keep]
    p = position.astype(f32)
    ex = p[rows, 0] - p[cols, 0]
    ey = p[rows, 1] - p[cols, 1]
    d = np.sqrt(ex * ex + ey * ey) / h.astype(f32)[rows]
    out = np.full(n, f32(2.0), f32)
    np.minimum.at(out, rows, d.astype(f32))
    return out


def colors(fields: Dict[str, np.ndarray], attribute: str, flags: int, stops, rest_density, maximum_surface_distance,
           neighbors=None) -> np.ndarray:
    """The colour of every particle (reference order) -> uint8[n, 3].  `fields`: host downloads; `stops`: the sph_render_params
    stops (ignored for the attributes without a map); `neighbors`: (offsets, indices) for MinDistanceToNeighbor."""
    from adaptive_sph_amd import ffi
    n = fields["mass"].shape[0]
    rho0 = f32(rest_density)
    out = np.zeros((n, 3), np.uint8)
    if attribute == "Aii":
        out[:] = cmap_get(stops, fields["aii"])
    elif attribute == "Distance":
        if flags & ffi.RENDER_FROM_STASH:
            d = fields["stash"].astype(f32)
        else:
            d = fields["level_estimation"].astype(f32).copy()
            d[np.isnan(d)] = -f32(maximum_surface_distance)
        out[:] = cmap_get(stops, d)
    elif attribute == "Pressure":
        p = fields["pressure"].astype(f32)
        pos = p[p > 0]
        mx = f32(pos.max()) if pos.size else f32(0.0)
        out[:] = cmap_get([(0.0, 1.0, 1.0, 1.0), (f32(mx * f32(0.9)), 1.0, 0.0, 0.0)], p)
    elif attribute == "Velocity":
        v = fields["velocity"].astype(f32)
        out[:] = cmap_get(stops, np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]))
    elif attribute == "Density":
        out[:] = cmap_get(stops, fields["density"].astype(f32) / rho0)
    elif attribute == "NeighborCount":
        base = f32(f32(ETA * f32(2.0)) * f32(ETA * f32(2.0)))
        out[:] = cmap_get(stops, fields["neighbor_count"].astype(f32) - base)
    elif attribute == "RandomColor":
        hs = np.array([rust_default_hash_usize(i) & 0xffffff for i in range(n)], np.uint64)
        out[:, 0], out[:, 1], out[:, 2] = hs & 0xff, (hs >> 8) & 0xff, (hs >> 16) & 0xff
    elif attribute == "ConstantField":
        out[:] = cmap_get(stops, fields["constant_field"])
    elif attribute == "MinDistanceToNeighbor":
        off, idx = neighbors
        out[:] = cmap_get(stops, min_distance_to_neighbor(fields["position"], fields["h2"], off, idx))
    elif attribute == "ParticleSizeClass":
        table = np.array([[0, 0, 255], [128, 128, 255], [255, 255, 255], [255, 128, 128], [255, 0, 0]], np.uint8)
        out[:] = table[np.minimum(fields["particle_size_class"].astype(np.int64), 4)]
    elif attribute == "SingleColor":
        out[:] = (80, 140, 255)
    elif attribute == "SourceTerm":
        out[:] = cmap_get(stops, fields["ppe_source_term"])
    else:
        raise ValueError(attribute)
    show_surface = bool(flags & ffi.RENDER_SHOW_SURFACE)
    if show_surface:
        out[fields["flag_insufficient_neighs"].astype(bool)] = (0, 255, 0)
        out[fields["flag_is_fluid_surface"].astype(bool)] = (255, 0, 0)
    if flags & ffi.RENDER_SHOW_NEIGHBORHOOD_REDUCED:
        out[fields["flag_neighborhood_reduced"].astype(bool)] = (0, 255, 0)
    return out


def radii(mass, rest_density) -> np.ndarray:
    """sphere_volume_to_radius(m / rho0) = sqrt((m / rho0) * FRAC_1_PI)."""
    return np.sqrt((np.asarray(mass, f32) / f32(rest_density)) * FRAC_1_PI)


def interpolate(p_after, p_before, alpha) -> np.ndarray:
    a = f32(alpha)
    return a * np.asarray(p_after, f32) + (f32(1.0) - a) * np.asarray(p_before, f32)


# ---- rasteriser -----------------------------------------------------------------------------------------------------------
class Frame:
    def __init__(self, width: int, height: int, supersample: int, zoom_out: float, segments=(), line_width: float = 0.005):
        self.w, self.h, self.s = int(width), int(height), int(supersample)
        self.ws, self.hs = self.w * self.s, self.h * self.s
        self.scale = f32(min(self.w, self.h) * self.s) / (f32(2.0) * f32(zoom_out))
        self.cx, self.cy = f32(self.ws) * f32(0.5), f32(self.hs) * f32(0.5)
        self.hw = (f32(line_width) * f32(0.5)) * self.scale
        seg = np.asarray(segments, f32).reshape(-1, 4)
        self.seg = np.stack([self.cx + seg[:, 0] * self.scale, self.cy - seg[:, 1] * self.scale,
                             self.cx + seg[:, 2] * self.scale, self.cy - seg[:, 3] * self.scale], axis=1).astype(f32)

    def discs(self, position, r):
        p = np.asarray(position, f32)
        r = np.asarray(r, f32)
        px = self.cx + p[:, 0] * self.scale
        py = self.cy - p[:, 1] * self.scale
        ro = (r * f32(1.05)) * self.scale
        ri = (r * f32(0.95)) * self.scale
        return px, py, ro, ri

    def keys(self, position, r) -> np.ndarray:
        """uint32[HS, WS]: 1 + the largest reference index whose outer disc covers the sample, 0 for none."""
        px, py, ro, _ = self.discs(position, r)
        keys = np.zeros(self.hs * self.ws, np.uint32)
        with np.errstate(invalid="ignore", over="ignore"):
            ok = (ro > 0) & (np.abs(px) < f32(1e30)) & (np.abs(py) < f32(1e30)) & (ro < f32(1e30))
            x0 = np.maximum(np.floor(px - ro) - 1, 0)
            x1 = np.minimum(np.ceil(px + ro) + 1, self.ws - 1)
            y0 = np.maximum(np.floor(py - ro) - 1, 0)
            y1 = np.minimum(np.ceil(py + ro) + 1, self.hs - 1)
        ok &= (x0 <= x1) & (y0 <= y1)
        idx = np.nonzero(ok)[0]
        x0, x1, y0, y1 = (a[idx].astype(np.int64) for a in (x0, x1, y0, y1))
        ext = np.maximum(x1 - x0, y1 - y0) + 1
        ro2 = ro * ro
        # particles grouped by the extent of their box: one vectorised pass per sample offset within it
        for e in np.unique(ext):
            g = ext == e
            gi, gx0, gx1, gy0, gy1 = idx[g], x0[g], x1[g], y0[g], y1[g]
            for dy in range(int(e)):
                for dx in range(int(e)):
                    sx, sy = gx0 + dx, gy0 + dy
                    m = (sx <= gx1) & (sy <= gy1)
                    if not m.any():
                        continue
                    ii, sxm, sym = gi[m], sx[m], sy[m]
                    du = (sxm.astype(f32) + f32(0.5)) - px[ii]
                    dv = (sym.astype(f32) + f32(0.5)) - py[ii]
                    cov = du * du + dv * dv < ro2[ii]
                    if cov.any():
                        np.maximum.at(keys, sym[cov] * self.ws + sxm[cov], (ii[cov] + 1).astype(np.uint32))
        return keys.reshape(self.hs, self.ws)

    def on_boundary(self, sx, sy) -> np.ndarray:
        u = sx.astype(f32) + f32(0.5)
        v = sy.astype(f32) + f32(0.5)
        hw2 = self.hw * self.hw
        hit = np.zeros(u.shape, bool)
        for ax, ay, bx, by in self.seg:
            ex, ey = bx - ax, by - ay
            wx, wy = u - ax, v - ay
            t = wx * ex + wy * ey
            L2 = ex * ex + ey * ey
            c = wx * ey - wy * ex
            hit |= (t >= 0) & (t <= L2) & (c * c < hw2 * L2)
        return hit

    def resolve(self, keys, position, r, rgb) -> np.ndarray:
        """uint8[H, W, 3] from the sample keys: winner's colour inside 0.95 r, black in the stroke band, else boundary or white."""
        px, py, _, ri = self.discs(position, r)
        sy, sx = np.mgrid[0:self.hs, 0:self.ws]
        k = keys.astype(np.int64)
        samples = np.full((self.hs, self.ws, 3), 255, np.uint32)
        cov = k > 0
        w = k[cov] - 1
        du = (sx[cov].astype(f32) + f32(0.5)) - px[w]
        dv = (sy[cov].astype(f32) + f32(0.5)) - py[w]
        fill = du * du + dv * dv < ri[w] * ri[w]
        col = np.where(fill[:, None], np.asarray(rgb, np.uint32)[w], 0)
        samples[cov] = col
        if self.seg.shape[0]:
            bnd = ~cov & self.on_boundary(sx, sy)
            samples[bnd] = 0
        ss = self.s * self.s
        acc = samples.reshape(self.h, self.s, self.w, self.s, 3).sum(axis=(1, 3))
        return ((acc + ss // 2) // ss).astype(np.uint8)

    def render(self, position, r, rgb) -> np.ndarray:
        return self.resolve(self.keys(position, r), position, r, rgb)
