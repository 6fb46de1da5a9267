"""include/sph_wall_load.h restated in numpy and Python ints: the boundary entries in np.float32, one operation at a time and lane for
lane; the terms as elementwise f64 operations in the header's order; the fixed-point integers, sums as Python ints; the keys, the bins,
the exponents, the offender and its sentence, the result's bytes.  Test infrastructure: the expectation every wall-load test compares the
library with, bit for bit -- and, through tests/test_wall_load_host.py, the oracle's own boundary entries and boundary pressure force."""
import math
import struct

import numpy as np

from tests.ledger_reference import MAX_EXP, MIN_EXP, NO_ID, NONE, Particles, exponent_of_bits, ord_f32, polygon_probe, resolve, unord  # noqa: F401

MAX_ELEMENTS, N_SUMS, MAX_BINS, BIN_SHIFT, MAX_BINNED = 8, 4, 4096, 40, 2 ** 23
SUMS = ["force_x", "force_y", "torque", "normal"]
FORCE_X, FORCE_Y, TORQUE, NORMAL = range(4)
BAD_M, BAD_X, BAD_Y, BAD_H, BAD_RHO, BAD_P, BAD_RHO_SIGN, BAD_H_SIGN, BAD_TERM = 1, 2, 3, 4, 5, 6, 7, 8, 16
INPUT_NAMES = ["mass", "x", "y", "smoothing length", "density", "pressure"]
PENALTY = {"None": 0, "Linear": 1, "Quadratic1": 2, "Quadratic2": 3}
LUT_N = 10001
f32 = np.float32


class Wall:
    """What the entries depend on besides the particles: the boundary (a list of (dir_x, dir_y, delta) planes, or an object with
    `.points`: the one polygon), the two lookup tables, and the parameters read."""

    def __init__(self, boundary, lam_lut, dlam_lut, penalty=0, sdf_gradient_eps=0.001, rest_density=1.0, symmetric=False):
        self.boundary = boundary
        self.points = getattr(boundary, "points", None)
        self.planes = [] if self.points is not None else [tuple(f32(v) for v in pl) for pl in boundary]
        self.n_elements = 1 if self.points is not None else len(self.planes)
        self.lam, self.dlam = np.asarray(lam_lut, f32), np.asarray(dlam_lut, f32)
        assert len(self.lam) == LUT_N and len(self.dlam) == LUT_N
        self.penalty = PENALTY[penalty] if isinstance(penalty, str) else int(penalty)
        self.eps, self.rest, self.symmetric = f32(sdf_gradient_eps), f32(rest_density), bool(symmetric)

    @classmethod
    def of(cls, boundary, luts, p, **kw):
        """From the ffi parameters `p` of a step."""
        return cls(boundary, luts[0], luts[1], int(p.boundary_penalty_term), float(p.sdf_gradient_eps), float(p.rest_density),
                   int(p.operator_discretization) == 1, **kw)

    def probe(self, k, x, y):
        if self.points is not None:
            return polygon_probe(self.points, x, y)
        dx, dy, delta = self.planes[k]
        return ((dx * x + dy * y) + delta).astype(f32)


def lut_get(data, x):
    """LookupTable1D::get over (-1, 1, 10000); -1 <= x < 1"""
    fidx = (x - f32(-1.0)) * f32(0.5) * f32(10000.0)
    fl = np.floor(fidx)
    interp = fidx - fl
    idx = fl.astype(np.int64)
    last = idx + 1 >= LUT_N
    nxt = np.where(last, idx, idx + 1)
    return np.where(last, data[idx], data[idx] * (f32(1.0) - interp) + data[nxt] * interp).astype(f32)


def entries(wall, x, y, h):
    """Per element k a dict of arrays over ALL the particles given: has (bool: the particle has an entry), d, nx, ny, gx, gy (f32; only
    meaningful where has).  sph_wall_load.h: THE ENTRY, steps 1 to 6."""
    x, y, h = (np.asarray(a, f32) for a in (x, y, h))
    one, zero = f32(1.0), f32(0.0)
    out = []
    with np.errstate(all="ignore"):
        sr = h * f32(2.0)
        eps = wall.eps
        inv_2eps = one / (f32(2.0) * eps)
        for k in range(wall.n_elements):
            d = (wall.probe(k, x, y) / sr).astype(f32)
            near = d < one
            gx = (wall.probe(k, x + eps, y) - wall.probe(k, x - eps, y)) * inv_2eps
            gy = (wall.probe(k, x, y + eps) - wall.probe(k, x, y - eps)) * inv_2eps
            gn = np.sqrt(gx * gx + gy * gy)
            has = near & (gn >= f32(0.00001))
            nx, ny = gx / gn, gy / gn
            if wall.penalty == 0:
                pen, dpen = np.full_like(d, one), np.full_like(d, zero)
            elif wall.penalty == 1:
                pen, dpen = one - d, np.full_like(d, -one)
            elif wall.penalty == 2:
                pen = np.where(d > zero, one, np.where(d > -one, f32(0.5) * d * d + one, f32(0.5) - d))
                dpen = np.where(d > zero, zero, np.where(d > -one, d, -one))
            else:
                pen = np.where(d > zero, one, np.where(d > f32(-0.5), d * d + one, f32(0.75) - d))
                dpen = np.where(d > zero, zero, np.where(d > f32(-0.5), f32(2.0) * d, -one))
            pen, dpen = pen.astype(f32), dpen.astype(f32)
            inside = has & (d > -one)                                      # the table's range: -1 < d < 1
            dc = np.where(inside, d, zero).astype(f32)
            lam = np.where(inside, lut_get(wall.lam, dc), one).astype(f32)
            dlam = np.where(inside, lut_get(wall.dlam, dc), zero).astype(f32)
            s = dpen * lam + pen * dlam
            out.append({"has": has, "d": d, "nx": nx.astype(f32), "ny": ny.astype(f32), "gx": (nx / sr * s).astype(f32), "gy": (ny / sr * s).astype(f32),
                        "lam": (lam * pen).astype(f32)})
    return out


def coefficient(wall, p, rho):
    """THE COEFFICIENT, f32"""
    with np.errstate(all="ignore"):
        p, rho = np.asarray(p, f32), np.asarray(rho, f32)
        p_ib = p if wall.symmetric else np.zeros_like(p)
        return (wall.rest * (p / (rho * rho) + p_ib / (wall.rest * wall.rest))).astype(f32)


def terms(m, c, x, y, e):
    """float64[4, n]: fx, fy, tq, fn of entry arrays e"""
    D = lambda a: np.asarray(a, f32).astype(np.float64)   # noqa: E731
    with np.errstate(all="ignore"):
        mc = D(m) * D(c)
        fx, fy = mc * D(e["gx"]), mc * D(e["gy"])
        return np.stack([fx, fy, D(x) * fy - D(y) * fx, -(fx * D(e["nx"]) + fy * D(e["ny"]))])


def input_reasons(P):
    bad = np.zeros(len(P), np.int64)

    def mark(fails, code):
        bad[(bad == 0) & fails] = code

    for a, code in ((P.m, BAD_M), (P.x, BAD_X), (P.y, BAD_Y), (P.h, BAD_H), (P.rho, BAD_RHO), (P.p, BAD_P)):
        mark(~np.isfinite(a), code)
    mark(~(P.rho > 0), BAD_RHO_SIGN)
    mark(~(P.h > 0), BAD_H_SIGN)
    return bad


def sentence(first_bad, exps):
    i, why = first_bad >> 8, first_bad & 0xFF
    if BAD_M <= why <= BAD_P:
        return f"wall load: the {INPUT_NAMES[why - BAD_M]} is not finite (particle i={i})"
    if why == BAD_RHO_SIGN:
        return f"wall load: the density is not positive (particle i={i}; before the first step the density is 0: the load exists behind sph_step)"
    if why == BAD_H_SIGN:
        return f"wall load: the smoothing length is not positive (particle i={i})"
    k, s = divmod(why - BAD_TERM, N_SUMS)
    if exps[k][s] is None:
        return f"wall load: the term of sum {s} ({SUMS[s]}) at element {k} is not finite (particle i={i})"
    return f"wall load: the term of sum {s} ({SUMS[s]}) at element {k} is not finite or not below 2^exponent = 2^{exps[k][s]} (particle i={i})"


def inv_ds_of(s_lo, s_hi, B):
    """(float)B / (s_hi - s_lo), f32"""
    return f32(B) / (f32(s_hi) - f32(s_lo))


def bin_of(wall, k, x, y, s_lo, inv_ds, B):
    """int64[n]: the bin of an entry of plane k at (x, y), -1 where it is not binned"""
    dx, dy, _ = wall.planes[k]
    with np.errstate(all="ignore"):
        s = ((-dy) * np.asarray(x, f32) + dx * np.asarray(y, f32)).astype(f32)
        fb = np.floor((s - f32(s_lo)) * f32(inv_ds))
    ok = (fb >= 0) & (fb < f32(B))
    return np.where(ok, np.where(ok, fb, 0).astype(np.int64), -1), s


def _norm_exps(exps, E):
    out = [[None] * N_SUMS for _ in range(MAX_ELEMENTS)]
    for k in range(min(E, len(exps) if exps is not None else 0)):
        if exps[k] is not None:
            out[k] = list(exps[k])
    return out


def wall_load(P, wall, bins=0, ranges=None, exps=None):
    """sph_wall_load_compute over the particles P (ledger_reference.Particles: m, x, y, h, rho, p, ids):
    ("ok", result dict, profile int64[E, bins] or None) or ("refused", sentence, None).
    ranges: per element None or (s_lo, s_hi[, B]); exps: per element None or four ints / None."""
    E = wall.n_elements
    exps = _norm_exps(exps, E)
    rng = []
    for k in range(E):
        r = None if ranges is None or k >= len(ranges) or bins == 0 else ranges[k]
        rng.append(None if r is None or (len(r) > 2 and r[2] == 0) else (f32(r[0]), f32(r[1]), int(r[2]) if len(r) > 2 else int(bins)))
    result = {"n_elements": E, "bins": int(bins) if E else 0, "n": len(P) if E else 0, "elements": []}
    if E == 0:
        return "ok", result, None
    bad = input_reasons(P)
    ok = np.flatnonzero(bad == 0)
    Q = P.subset(ok)
    ent = entries(wall, Q.x, Q.y, Q.h)
    c = coefficient(wall, Q.p, Q.rho)
    t = [terms(Q.m, c, Q.x, Q.y, e) for e in ent]
    tbad = np.zeros(len(Q), np.int64)
    for k in range(E):
        for s in range(N_SUMS):
            limit = np.inf if exps[k][s] is None else 2.0 ** exps[k][s]
            fails = ent[k]["has"] & ~(np.abs(t[k][s]) < limit)
            tbad[(tbad == 0) & fails] = BAD_TERM + k * N_SUMS + s
    bad[ok] = tbad
    if bad.any():
        j = np.flatnonzero(bad)
        j = j[np.argmin(P.ids[j])]
        return "refused", sentence((int(P.ids[j]) << 8) | int(bad[j]), exps), None
    profile = np.zeros((E, bins), np.int64) if bins > 0 else None
    for k in range(E):
        has = np.flatnonzero(ent[k]["has"])
        tk = t[k][:, has]
        el = {"n_entries": len(has), "n_wet": int((Q.p[has] > 0).sum()), "n_unbinned": 0, "inv_ds": 0.0, "n_bins": 0}
        used = []
        for s in range(N_SUMS):
            if exps[k][s] is not None:
                used.append(exps[k][s])
                continue
            bits = int(np.abs(tk[s]).view(np.uint64).max()) if len(has) else 0
            e = max(exponent_of_bits(bits), MIN_EXP)
            if e > MAX_EXP:
                return "refused", f"wall load: sum {s} ({SUMS[s]}) at element {k} needs the exponent {e} (at most {MAX_EXP})", None
            used.append(e)
        el["exponent"] = used
        el["raw"] = [sum(int(v) for v in np.trunc(tk[s] * 2.0 ** (60 - used[s])).astype(np.int64)) for s in range(N_SUMS)]
        el["sum"] = [resolve(el["raw"][s], used[s]) for s in range(N_SUMS)]
        if len(has):
            o = ord_f32(Q.p[has])
            key = max((int(a) << 32) | (NO_ID - int(i)) for a, i in zip(o, Q.ids[has]))
            el["max_pressure"] = (unord(key >> 32), NO_ID - (key & 0xFFFFFFFF))
        else:
            el["max_pressure"] = (0.0, NO_ID)
        if rng[k] is not None:
            s_lo, s_hi, B = rng[k]
            inv_ds = inv_ds_of(s_lo, s_hi, B)
            if len(has) >= MAX_BINNED:
                return "refused", (f"wall load: element {k} has {len(has)} entries: with bins fewer than 2^23 = {MAX_BINNED} (the profile's 64-bit words hold that "
                                   "many terms below 2^40)"), None
            b, _ = bin_of(wall, k, Q.x[has], Q.y[has], s_lo, inv_ds, B)
            q = np.trunc(tk[NORMAL] * 2.0 ** (BIN_SHIFT - used[NORMAL])).astype(np.int64)
            np.add.at(profile[k], b[b >= 0], q[b >= 0])
            el.update(n_unbinned=int((b < 0).sum()), inv_ds=float(inv_ds), n_bins=B)
            el["unbinned_terms"] = int(sum(int(v) for v in q[b < 0]))     # (not part of the result: for the tests' own sums)
        result["elements"].append(el)
    return "ok", result, profile


def result_bytes(r):
    """The 1232 bytes of the sph_wall_load_result the dict stands for."""
    out = struct.pack("<IiQ", r["n_elements"], r["bins"], r["n"])
    for el in r["elements"]:
        out += struct.pack("<4i", *el["exponent"])
        for q in el["raw"]:
            lo = q & (2 ** 64 - 1)
            out += struct.pack("<Qq", lo, (q - lo) >> 64)
        out += struct.pack("<4d", *el["sum"])
        out += struct.pack("<QQQ", el["n_entries"], el["n_wet"], el["n_unbinned"])
        out += struct.pack("<fI", *el["max_pressure"])
        out += struct.pack("<fi", el["inv_ds"], el["n_bins"])
    return out + bytes(152 * (MAX_ELEMENTS - len(r["elements"])))


def profile_bytes(profile, E, bins):
    """The E x bins int64 words the call writes."""
    return b"" if profile is None else np.ascontiguousarray(profile[:E, :bins], np.int64).tobytes()


def resolve_bin(word, e_normal):
    return math.ldexp(float(word), e_normal - BIN_SHIFT)
