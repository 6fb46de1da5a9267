"""TEST INFRASTRUCTURE: a numpy restatement of the device's probe sets (include/sph_probe.h, adaptive_sph_amd/csrc/sph_probe.hip).

The per-particle terms, the exponents and the precondition check are tests/sample_reference.py's, unchanged; this adds the sums at
arbitrary points -- brute force over (particle, point) pairs, every operation one float32 operation in the header's order, the sums in
int64 -- and the tracer step.  Nothing here is imported by the product."""
import numpy as np

from tests.sample_reference import TWO32, Particles, exponents, f32, first_offender  # noqa: F401  (re-exported for the tests)


def raw_at_points(p, exps, PX, PY, chunk=64):
    """-> (int64[C+1, n_points], footprint[n_particles], touched[n_points]): the sums over all particles at the points (PX[k], PY[k]),
    how many points each particle touches, and which points at least one particle touches."""
    PX, PY = np.asarray(PX, f32), np.asarray(PY, f32)
    C = len(p.a)
    out = np.zeros((C + 1, len(PX)), np.int64)
    foot = np.zeros(p.n, np.int64)
    touched = np.zeros(len(PX), bool)
    scale = [np.ldexp(f32(1.0), 32 - int(e)) for e in exps]
    with np.errstate(all="ignore"):
        for s in range(0, p.n, chunk):
            sl = slice(s, min(s + chunk, p.n))
            dx = PX[None, :] - p.x[sl, None]
            dy = PY[None, :] - p.y[sl, None]
            r = np.sqrt(dx * dx + dy * dy)
            q = r / (f32(2.0) * p.h[sl])[:, None]
            touch = q < f32(1.0)
            ka = f32(6.0) * (q * q * q - q * q) + f32(1.0)
            v = f32(1.0) - q
            kb = f32(2.0) * (v * v * v)
            k = np.where(q < f32(0.5), ka, kb)
            W = p.norm[sl, None] * k
            w = p.V[sl, None] * W
            assert w.dtype == f32
            foot[sl] = touch.sum(axis=1)
            touched |= touch.any(axis=0)
            out[0] += np.where(touch, np.trunc(w * TWO32), f32(0)).astype(np.int64).sum(axis=0)
            for c in range(C):
                t = w * p.a[c, sl, None]
                out[c + 1] += np.where(touch, np.trunc(t * scale[c]), f32(0)).astype(np.int64).sum(axis=0)
    return out, foot, touched


def advect(raw, exps, PX, PY, dt, min_weight):
    """The tracer step: raw int64[3, n] (weight, x, y sums), their two exponents -> (X', Y', moved[n])."""
    PX, PY = np.asarray(PX, f32), np.asarray(PY, f32)
    raw = np.asarray(raw, np.int64)
    dt = f32(dt)
    with np.errstate(all="ignore"):
        weight = (raw[0].astype(np.float64) * 2.0 ** -32).astype(f32)
        ux = (raw[1].astype(np.float64) * 2.0 ** (int(exps[0]) - 32)).astype(f32) / weight
        uy = (raw[2].astype(np.float64) * 2.0 ** (int(exps[1]) - 32)).astype(f32) / weight
        X = (PX + (dt * ux).astype(f32)).astype(f32)
        Y = (PY + (dt * uy).astype(f32)).astype(f32)
        moved = (weight >= f32(min_weight)) & np.isfinite(X) & np.isfinite(Y)
    return np.where(moved, X, PX).astype(f32), np.where(moved, Y, PY).astype(f32), moved


def read_vtk_points(path):
    """An independent reader of what write_vtk_points writes: (float32[n, 2] points, {name: array}); the z of every point must be 0 and
    the vertices must be one cell per point in order."""
    blob = open(path, "rb").read()
    pos = 0

    def line():
        nonlocal pos
        end = blob.index(b"\n", pos)
        out = blob[pos:end].decode()
        pos = end + 1
        return out

    def skip_newline():
        nonlocal pos
        assert blob[pos:pos + 1] == b"\n"
        pos += 1

    head = [line() for _ in range(4)]
    assert head[0] == "# vtk DataFile Version 4.2" and head[2] == "BINARY" and head[3] == "DATASET POLYDATA", head
    words = line().split()
    assert words[0] == "POINTS" and words[2] == "float"
    n = int(words[1])
    pts = np.frombuffer(blob, ">f4", 3 * n, pos).astype(np.float32).reshape(n, 3)
    pos += 12 * n
    skip_newline()
    assert line() == f"VERTICES {n} {2 * n}"
    verts = np.frombuffer(blob, ">i4", 2 * n, pos).reshape(n, 2)
    pos += 8 * n
    assert (verts[:, 0] == 1).all() and np.array_equal(verts[:, 1], np.arange(n)) and not pts[:, 2].any()
    skip_newline()
    assert line() == f"POINT_DATA {n}"
    data = {}
    while pos < len(blob):
        words = line().split()
        assert words[0] == "SCALARS" and words[3] == "1" and line() == "LOOKUP_TABLE default", words
        kind = {"float": ">f4", "int": ">i4"}[words[2]]
        data[words[1]] = np.frombuffer(blob, kind, n, pos).astype(kind[1:])
        pos += 4 * n
        skip_newline()
    return pts[:, :2].copy(), data
