"""TEST INFRASTRUCTURE: a numpy restatement of the device's field sampling (include/sph_sample.h, adaptive_sph_amd/csrc/sph_sample.hip).

Brute force over (particle, sample) pairs, every operation one float32 operation in the header's order, the sums in int64: what the
device accumulates with integer atomics in whatever order, this adds in index order -- the planes must agree bit for bit.  Nothing
here is imported by the product."""
import numpy as np

f32 = np.float32
PI_F = f32(3.14159274101257324219)
TWO32 = f32(4294967296.0)

# channel name -> (field a `fields` dict holds, component)
CHANNELS = {"density": ("density", None), "pressure": ("pressure", None), "velocity_x": ("velocity", 0), "velocity_y": ("velocity", 1),
            "constant_field": ("constant_field", None), "level_estimation": ("level_estimation", None)}
BAD_H, BAD_V, BAD_VNORM, BAD_CHANNEL = 1, 2, 3, 4


def centers(nx, ny, origin, spacing):
    """(X[nx], Y[ny]): X = origin_x + ((float)sx + 0.5f) * spacing."""
    X = f32(origin[0]) + (np.arange(nx).astype(f32) + f32(0.5)) * f32(spacing)
    Y = f32(origin[1]) + (np.arange(ny).astype(f32) + f32(0.5)) * f32(spacing)
    return X.astype(f32), Y.astype(f32)


class Particles:
    """The per-particle terms of sph_sample.h from host arrays in reference order: x, y, h, V, norm, and a[C, n]."""

    def __init__(self, fields, channels, rest_density, maximum_surface_distance=0.0, volume="density"):
        pos = np.asarray(fields["position"], f32).reshape(-1, 2)
        self.x, self.y = pos[:, 0].copy(), pos[:, 1].copy()
        self.h = np.asarray(fields["h2"], f32)
        m = np.asarray(fields["mass"], f32)
        with np.errstate(all="ignore"):
            self.V = (m / f32(rest_density)).astype(f32) if volume == "rest" else (m / np.asarray(fields["density"], f32)).astype(f32)
            self.norm = (f32(10.0) / ((f32(7.0) * PI_F) * (self.h * self.h))).astype(f32)
        a = []
        for name in channels:
            field, comp = CHANNELS[name]
            v = np.asarray(fields[field], f32)
            v = v.reshape(-1, 2)[:, comp] if comp is not None else v
            if field == "level_estimation":
                v = np.where(np.isnan(v), -f32(maximum_surface_distance), v)   # FluidInterior: the renderer's DISTANCE rule
            a.append(v.astype(f32))
        self.a = np.stack(a) if a else np.zeros((0, len(self.x)), f32)
        self.n = len(self.x)

    def subset(self, idx):
        q = object.__new__(Particles)
        q.x, q.y, q.h, q.V, q.norm, q.a = self.x[idx], self.y[idx], self.h[idx], self.V[idx], self.norm[idx], self.a[:, idx]
        q.n = len(q.x)
        return q


def max_abs(p):
    """max_j |a_j| per channel (float32[C]; 0 for no particles)."""
    return np.array([np.abs(p.a[c]).max() if p.n else f32(0) for c in range(len(p.a))], f32)


def exponent_of(m):
    """The smallest e with m < 2^e, 0 for m == 0 (frexp: m = f 2^e with 0.5 <= f < 1)."""
    return int(np.frexp(f32(m))[1]) if m > 0 else 0


def exponents(p, lo=-64):
    return [max(exponent_of(m), lo) for m in max_abs(p)]


def first_offender(p, exps=None):
    """(reference index, reason) of the smallest index that fails a precondition, or None.  `exps`: the explicit exponents (None per
    channel, or altogether: only finiteness is asked of that channel)."""
    with np.errstate(all="ignore"):
        ok_h = np.isfinite(p.h) & (p.h > 0)
        ok_v = np.isfinite(p.V) & (p.V >= 0)
        ok_vn = (p.V * p.norm).astype(f32) < f32(1048576.0)
        checks = [(~ok_h, BAD_H), (~ok_v, BAD_V), (~ok_vn, BAD_VNORM)]
        for c in range(len(p.a)):
            lim = f32(np.inf) if exps is None or exps[c] is None else np.ldexp(f32(1.0), int(exps[c]))
            checks.append((~(np.abs(p.a[c]) < lim), BAD_CHANNEL + c))
        bad = np.zeros(p.n, np.int64)
        for cond, code in checks:   # a particle reports its first failing check, in this order
            bad = np.where((bad == 0) & cond, code, bad)
    idx = np.flatnonzero(bad)
    return (int(idx[0]), int(bad[idx[0]])) if len(idx) else None


def _reach(X, x, h):
    """The slice of the ascending points X within the largest support radius (and 5 % of it, and a rounding allowance) of some x."""
    x, h = x.astype(np.float64), h.astype(np.float64)
    ok = np.isfinite(x) & np.isfinite(h)
    if not ok.all() or len(X) == 0:   # (a particle that is not finite: no shortcut)
        return slice(0, len(X))
    slack = 0.1 * h.max() + 1e-4 * (1.0 + float(np.abs(X).max()))
    lo = np.searchsorted(X.astype(np.float64), (x - 2.0 * h).min() - slack, "left")
    hi = np.searchsorted(X.astype(np.float64), (x + 2.0 * h).max() + slack, "right")
    return slice(int(lo), int(hi))


def raw_planes(p, exps, X, Y, chunk=96):
    """-> (int64[C+1, len(Y), len(X)], footprint[n]): the sums over all particles at the points X x Y, and how many of the points each
    particle touches."""
    C = len(p.a)
    out = np.zeros((C + 1, len(Y), len(X)), np.int64)
    foot = np.zeros(p.n, np.int64)
    scale = [np.ldexp(f32(1.0), 32 - int(e)) for e in exps]
    with np.errstate(all="ignore"):
        for s in range(0, p.n, chunk):
            sl = slice(s, min(s + chunk, p.n))
            # (the part of X x Y the chunk can reach, a superset taken in float64 with slack: the pairs left out have q > 1)
            ix, iy = _reach(X, p.x[sl], p.h[sl]), _reach(Y, p.y[sl], p.h[sl])
            out_c, X_c, Y_c = out[:, iy, ix], X[ix], Y[iy]
            dx = X_c[None, None, :] - p.x[sl, None, None]
            dy = Y_c[None, :, None] - p.y[sl, None, None]
            r = np.sqrt(dx * dx + dy * dy)
            q = r / (f32(2.0) * p.h[sl])[:, None, None]
            touch = q < f32(1.0)
            ka = f32(6.0) * (q * q * q - q * q) + f32(1.0)
            v = f32(1.0) - q
            kb = f32(2.0) * (v * v * v)
            k = np.where(q < f32(0.5), ka, kb)
            W = p.norm[sl, None, None] * k
            w = p.V[sl, None, None] * W
            assert w.dtype == f32
            foot[sl] = touch.sum(axis=(1, 2))
            out_c[0] += np.where(touch, np.trunc(w * TWO32), f32(0)).astype(np.int64).sum(axis=0)
            for c in range(C):
                t = w * p.a[c, sl, None, None]
                out_c[c + 1] += np.where(touch, np.trunc(t * scale[c]), f32(0)).astype(np.int64).sum(axis=0)
    return out, foot


def sample(fields, channels, rest_density, maximum_surface_distance, nx, ny, origin, spacing, volume="density", exps=None):
    """The whole call: (raw int64[C+1, ny, nx], exponents used, n_touching, (max_footprint, n_pairs))."""
    p = Particles(fields, channels, rest_density, maximum_surface_distance, volume)
    auto = exponents(p)
    used = [auto[c] if exps is None or exps[c] is None else int(exps[c]) for c in range(len(channels))]
    X, Y = centers(nx, ny, origin, spacing)
    raw, foot = raw_planes(p, used, X, Y)
    return raw, used, int((foot > 0).sum()), (int(foot.max()) if p.n else 0, int(foot.sum()))


def window_planes(p, exps, nx, ny, origin, spacing, window):
    """The windowed form: the raw planes at the samples [sx0, sx1) x [sy0, sy1) of the grid, from the particles that can reach the
    window only -- prefiltered in float64 by the distance of the particle to the window's centre against its support radius, the
    window's half diagonal and a spacing of slack (a superset; the predicate decides)."""
    sx0, sx1, sy0, sy1 = window
    X, Y = centers(nx, ny, origin, spacing)
    X, Y = X[sx0:sx1], Y[sy0:sy1]
    cx, cy = 0.5 * (float(X[0]) + float(X[-1])), 0.5 * (float(Y[0]) + float(Y[-1]))
    half = 0.5 * np.hypot(float(X[-1]) - float(X[0]), float(Y[-1]) - float(Y[0]))
    d = np.hypot(p.x.astype(np.float64) - cx, p.y.astype(np.float64) - cy)
    near = np.flatnonzero(~(d > 2.0 * p.h.astype(np.float64) * 1.001 + half + float(spacing)))
    return raw_planes(p.subset(near), exps, X, Y)[0]


def read_vtk_grid(path):
    """An independent reader of what write_vtk_grid writes: ((nx, ny), origin, spacing, {name: float32[ny, nx]}); VECTORS come back as
    <name>_x / <name>_y (their z must be 0)."""
    blob = open(path, "rb").read()
    pos = 0

    def line():
        nonlocal pos
        end = blob.index(b"\n", pos)
        out = blob[pos:end].decode()
        pos = end + 1
        return out

    head = [line() for _ in range(4)]
    assert head[0] == "# vtk DataFile Version 4.2" and head[2] == "BINARY" and head[3] == "DATASET STRUCTURED_POINTS", head
    nx, ny, nz = (int(v) for v in line().split()[1:])
    origin = tuple(float(v) for v in line().split()[1:])
    spacing = tuple(float(v) for v in line().split()[1:])
    assert nz == 1 and line() == f"POINT_DATA {nx * ny}"
    planes = {}
    while pos < len(blob):
        words = line().split()
        if words[0] == "SCALARS":
            assert words[2:] == ["float", "1"] and line() == "LOOKUP_TABLE default"
            planes[words[1]] = np.frombuffer(blob, ">f4", nx * ny, pos).astype(f32).reshape(ny, nx)
            pos += 4 * nx * ny
        else:
            assert words[0] == "VECTORS" and words[2] == "float", words
            v = np.frombuffer(blob, ">f4", 3 * nx * ny, pos).astype(f32).reshape(ny, nx, 3)
            pos += 12 * nx * ny
            assert not v[:, :, 2].any()
            planes[words[1] + "_x"], planes[words[1] + "_y"] = v[:, :, 0].copy(), v[:, :, 1].copy()
        assert blob[pos:pos + 1] == b"\n"
        pos += 1
    return (nx, ny), origin, spacing, planes
