"""include/sph_ledger.h restated in numpy and Python ints: the terms as elementwise f64 operations in the header's order, the fixed-point
integers, sums as Python ints, the keys, fold, compose, resolve, the offender and its sentence.  Test infrastructure: the expectation
every ledger test compares the library with, bit for bit."""
import math
import struct

import numpy as np

CARRIED, STEP, OUTSIDE = 1, 2, 4
ALL = CARRIED | STEP | OUTSIDE
N_SUMS, N_EXT = 9, 13
SUMS = ["mass", "momentum_x", "momentum_y", "moment_x", "moment_y", "kinetic", "angular", "volume", "compression"]
EXTREMES = ["max_speed2", "min_x", "max_x", "min_y", "max_y", "min_mass", "max_mass", "min_density", "max_density", "min_pressure", "max_pressure",
            "min_h", "max_h"]
MIN_EXP, MAX_EXP = -200, 200
NONE = 2 ** 64 - 1
NO_ID = 2 ** 32 - 1
BAD_M, BAD_X, BAD_Y, BAD_VX, BAD_VY, BAD_RHO, BAD_P, BAD_H, BAD_SPEED2, BAD_RHO_SIGN, BAD_TERM = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16
INPUT_NAMES = ["mass", "x", "y", "vx", "vy", "density", "pressure", "smoothing length"]
f32 = np.float32


def sum_mask(what):
    return (0x7F if what & CARRIED else 0) | (0x180 if what & STEP else 0)


def extreme_mask(what):
    return (0x7F if what & CARRIED else 0) | (0x1F80 if what & STEP else 0)


def is_max(k):
    return k % 2 == 0


class Particles:
    """The fields a ledger reads, float32, and the ids (reference indices / global ids), in any order."""

    def __init__(self, fields, ids=None, rest_density=1000.0):
        n = len(fields["mass"])
        z = np.zeros(n, f32)
        pos = np.asarray(fields["position"], f32).reshape(n, 2)
        vel = np.asarray(fields.get("velocity", np.zeros((n, 2))), f32).reshape(n, 2)
        self.m = np.asarray(fields["mass"], f32)
        self.x, self.y = pos[:, 0].copy(), pos[:, 1].copy()
        self.vx, self.vy = vel[:, 0].copy(), vel[:, 1].copy()
        self.rho = np.asarray(fields.get("density", z), f32)
        self.p = np.asarray(fields.get("pressure", z), f32)
        self.h = np.asarray(fields.get("h2", z), f32)
        self.ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
        self.rest = f32(rest_density)

    def subset(self, idx):
        """The particles whose POSITION in the arrays is in idx (ids travel with them)."""
        q = Particles.__new__(Particles)
        for k in ("m", "x", "y", "vx", "vy", "rho", "p", "h", "ids"):
            setattr(q, k, getattr(self, k)[idx])
        q.rest = self.rest
        return q

    def __len__(self):
        return len(self.m)


def terms(P, what):
    """float64[9, n]: sph_ledger.h's terms, one IEEE f64 operation each; 0 for a group that is not asked for."""
    with np.errstate(all="ignore"):
        t = np.zeros((N_SUMS, len(P)), np.float64)
        M = P.m.astype(np.float64)
        if what & CARRIED:
            X, Y, VX, VY = (a.astype(np.float64) for a in (P.x, P.y, P.vx, P.vy))
            t[0] = M
            t[1] = M * VX
            t[2] = M * VY
            t[3] = M * X
            t[4] = M * Y
            t[5] = 0.5 * (M * (VX * VX + VY * VY))
            t[6] = M * (X * VY - Y * VX)
        if what & STEP:
            RHO = P.rho.astype(np.float64)
            t[7] = M / RHO
            d = RHO - np.float64(P.rest)
            t[8] = np.where(d > 0.0, d, 0.0)
    return t


def speed2(P):
    with np.errstate(all="ignore"):
        return (P.vx * P.vx + P.vy * P.vy).astype(f32)   # two products and one sum, each rounded to f32


def reasons(P, what, exps=None):
    """uint8[n]: the first failing check of every particle (0: none).  exps: None, or one int / None per sum."""
    n = len(P)
    exps = [None] * N_SUMS if exps is None else list(exps)
    carried, step, outside = bool(what & CARRIED), bool(what & STEP), bool(what & OUTSIDE)
    checks = [(carried or step, P.m, BAD_M), (carried or outside, P.x, BAD_X), (carried or outside, P.y, BAD_Y), (carried, P.vx, BAD_VX),
              (carried, P.vy, BAD_VY), (step, P.rho, BAD_RHO), (step, P.p, BAD_P), (step, P.h, BAD_H)]
    bad = np.zeros(n, np.int64)

    def mark(fails, code):
        bad[(bad == 0) & fails] = code

    for on, a, code in checks:
        if on:
            mark(~np.isfinite(a), code)
    if carried:
        mark(~np.isfinite(speed2(P)), BAD_SPEED2)
    if step:
        mark(~(P.rho > 0), BAD_RHO_SIGN)
    with np.errstate(all="ignore"):
        t = np.abs(terms(P, what))
    for s in range(N_SUMS):
        if (sum_mask(what) >> s) & 1:
            limit = np.inf if exps[s] is None else 2.0 ** exps[s]
            mark(~(t[s] < limit), BAD_TERM + s)
    return bad


def ord_f32(a):
    b = np.asarray(a, f32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b ^ 0x80000000)


def unord(o):
    b = (o ^ 0x80000000) if (o & 0x80000000) else (~o & 0xFFFFFFFF)
    return float(np.array([b], np.uint32).view(f32)[0])


# ---- the boundary probe (sph_device.h: sdf_probe) -------------------------------------------------------------------------------
def polygon_tables(points):
    """sph_set_boundary_polygon's tables: points, normalised edge directions, pseudo normals, all f32."""
    px = np.array([p[0] for p in points], f32)
    py = np.array([p[1] for p in points], f32)
    ex, ey = np.roll(px, -1) - px, np.roll(py, -1) - py
    nn = np.sqrt(ex * ex + ey * ey)
    dx, dy = ex / nn, ey / nn
    nx, ny = -np.roll(dy, 1) + -dy, np.roll(dx, 1) + dx
    return px, py, dx, dy, nx, ny


def polygon_probe(points, x, y):
    """Sdf2D::probe as sph_device.h's polygon_probe computes it: f32, one operation at a time, vectorised over the particles."""
    px, py, dx, dy, nx, ny = polygon_tables(points)
    n = len(px)
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    min_d2 = np.full(len(x), np.inf, f32)
    is_line = np.zeros(len(x), bool)
    point_idx = np.zeros(len(x), np.int64)
    line_dist, pdx, pdy, pt_d2 = (np.zeros(len(x), f32) for _ in range(4))
    pt_d2[:] = np.inf
    with np.errstate(all="ignore"):
        for i in range(n):
            i1 = (i + 1) % n
            lx, ly = px[i1] - px[i], py[i1] - py[i]
            line_len_sq = f32(f32(lx * lx) + f32(ly * ly))
            qx, qy = x - px[i], y - py[i]
            proj = qx * dx[i] + qy * dy[i]
            on = (proj > 0) & (proj * proj < line_len_sq)
            d = qx * -dy[i] + qy * dx[i]
            d2 = d * d
            take = on & (d2 < min_d2)
            is_line[take] = True
            line_dist[take] = d[take]
            min_d2[take] = d2[take]
            c2 = qx * qx + qy * qy
            take = c2 < min_d2
            is_line[take] = False
            point_idx[take] = i
            pt_d2[take] = c2[take]
            pdx[take] = qx[take]
            pdy[take] = qy[take]
            min_d2[take] = c2[take]
        sign = np.where(nx[point_idx] * pdx + ny[point_idx] * pdy >= 0, f32(1), f32(-1))
        return np.where(is_line, line_dist, np.sqrt(pt_d2) * sign).astype(f32)


def outside(boundary, x, y):
    """bool[n]: min_k probe_k(x, y) < 0.  boundary: a list of (dir_x, dir_y, delta) planes (empty: no boundary), or an object with
    `.points` (the one polygon)."""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    pts = getattr(boundary, "points", None)
    if pts is not None:
        return polygon_probe(pts, x, y) < 0
    dist = np.full(len(x), np.inf, f32)
    with np.errstate(all="ignore"):
        for dx, dy, delta in boundary:
            dist = np.minimum(dist, (f32(dx) * x + f32(dy) * y) + f32(delta))
    return dist < 0


# ---- words, fold, sums, compose -------------------------------------------------------------------------------------------------
def empty_words():
    return (NONE, 0, 0, (0,) * N_SUMS, tuple(0 if is_max(k) else NONE for k in range(N_EXT)))


def words(P, what, exps=None, boundary=()):
    """sph_ledger_words of these particles as (first_bad, n, n_outside, max_bits[9], extreme[13]) of Python ints."""
    bad = reasons(P, what, exps)
    first = NONE
    if bad.any():
        k = np.flatnonzero(bad)
        j = k[np.argmin(P.ids[k])]
        first = (int(P.ids[j]) << 8) | int(bad[j])
    ok = P.subset(np.flatnonzero(bad == 0))
    t = np.abs(terms(ok, what))
    bits = tuple(int(t[s].view(np.uint64).max()) if len(ok) else 0 for s in range(N_SUMS))
    values = [speed2(ok), ok.x, ok.x, ok.y, ok.y, ok.m, ok.m, ok.rho, ok.rho, ok.p, ok.p, ok.h, ok.h]
    keys = []
    for k in range(N_EXT):
        if not ((extreme_mask(what) >> k) & 1) or not len(ok):
            keys.append(0 if is_max(k) else NONE)
            continue
        o = ord_f32(values[k])
        if is_max(k):
            keys.append(max((int(a) << 32) | (NO_ID - int(i)) for a, i in zip(o, ok.ids)))
        else:
            keys.append(min((int(a) << 32) | int(i) for a, i in zip(o, ok.ids)))
    n_out = int(outside(boundary, ok.x, ok.y).sum()) if (what & OUTSIDE) and len(ok) else 0
    return first, len(P), n_out, bits, tuple(keys)


def fold_only(all_words):
    f = list(empty_words())
    f[3], f[4] = list(f[3]), list(f[4])
    for w in all_words:
        f[0] = min(f[0], w[0])
        f[1] += w[1]
        f[2] += w[2]
        f[3] = [max(a, b) for a, b in zip(f[3], w[3])]
        f[4] = [(max if is_max(k) else min)(a, b) for k, (a, b) in enumerate(zip(f[4], w[4]))]
    return f[0], f[1], f[2], tuple(f[3]), tuple(f[4])


def exponent_of_bits(bits):
    m = struct.unpack("<d", struct.pack("<Q", bits))[0]
    return math.frexp(m)[1] if m > 0 else 0


def sentence(first_bad, exps):
    i, why = first_bad >> 8, first_bad & 0xFF
    if BAD_M <= why <= BAD_H:
        return f"ledger: the {INPUT_NAMES[why - BAD_M]} is not finite (particle i={i})"
    if why == BAD_SPEED2:
        return f"ledger: the squared speed vx * vx + vy * vy is not finite in f32 (particle i={i})"
    if why == BAD_RHO_SIGN:
        return f"ledger: the density is not positive (particle i={i}; before the first step the density is 0: step outputs exist behind sph_step)"
    s = why - BAD_TERM
    if exps[s] is None:
        return f"ledger: the term of sum {s} ({SUMS[s]}) is not finite (particle i={i})"
    return f"ledger: the term of sum {s} ({SUMS[s]}) is not finite or not below 2^exponent = 2^{exps[s]} (particle i={i})"


def fold(all_words, what, exps=None):
    """("ok", the exponents used (0 for a sum not asked for), folded words) or ("refused", sentence, folded words)"""
    exps = [None] * N_SUMS if exps is None else list(exps)
    f = fold_only(all_words)
    if f[0] != NONE:
        return "refused", sentence(f[0], exps), f
    used = []
    for s in range(N_SUMS):
        if not ((sum_mask(what) >> s) & 1):
            used.append(0)
        elif exps[s] is not None:
            used.append(exps[s])
        else:
            e = max(exponent_of_bits(f[3][s]), MIN_EXP)
            if e > MAX_EXP:
                return "refused", f"ledger: sum {s} ({SUMS[s]}) needs the exponent {e} (at most {MAX_EXP})", f
            used.append(e)
    return "ok", used, f


def sums(P, what, used):
    """The nine Python ints: sum_j (int64) trunc(t_j * 2^(60 - e_s)); 0 for a sum not asked for."""
    t = terms(P, what)
    out = []
    for s in range(N_SUMS):
        if not ((sum_mask(what) >> s) & 1):
            out.append(0)
            continue
        q = np.trunc(t[s] * 2.0 ** (60 - used[s])).astype(np.int64)
        out.append(sum(int(v) for v in q))
    return out


def resolve(q, e):
    return math.ldexp(float(q), e - 60)


def compose(all_words, all_sums, what, used):
    """The sph_ledger_result as a dict: what, exponent, n, n_outside, raw (ints), sum (floats), extreme [(value, id)]."""
    f = fold_only(all_words)
    assert f[0] == NONE
    raw = [sum(r[s] for r in all_sums) if (sum_mask(what) >> s) & 1 else 0 for s in range(N_SUMS)]
    exponent = [used[s] if (sum_mask(what) >> s) & 1 else 0 for s in range(N_SUMS)]
    ext = []
    for k in range(N_EXT):
        key = f[4][k]
        if not ((extreme_mask(what) >> k) & 1) or key == (0 if is_max(k) else NONE):
            ext.append((0.0, NO_ID))
        else:
            low = key & 0xFFFFFFFF
            ext.append((unord(key >> 32), NO_ID - low if is_max(k) else low))
    return {"what": what, "exponent": exponent, "n": f[1], "n_outside": f[2] if what & OUTSIDE else 0, "raw": raw,
            "sum": [resolve(raw[s], exponent[s]) for s in range(N_SUMS)], "extreme": ext}


def result_bytes(r):
    """The 376 bytes of the sph_ledger_result the dict stands for."""
    out = struct.pack("<I9iQQ", r["what"], *r["exponent"], r["n"], r["n_outside"])
    for q in r["raw"]:
        lo = q & (2 ** 64 - 1)
        out += struct.pack("<Qq", lo, (q - lo) >> 64)
    out += struct.pack("<9d", *r["sum"])
    for v, i in r["extreme"]:
        out += struct.pack("<fI", v, i)
    return out


def ledger(P, what=ALL, exps=None, boundary=(), parts=None):
    """The whole path over `parts` (lists of positions; default: one part): ("ok", result dict) or ("refused", sentence)."""
    parts = [np.arange(len(P))] if parts is None else parts
    ws = [words(P.subset(i), what, exps, boundary) for i in parts]
    kind, used, _ = fold(ws, what, exps)
    if kind != "ok":
        return kind, used
    return "ok", compose(ws, [sums(P.subset(i), what, used) for i in parts], what, used)
