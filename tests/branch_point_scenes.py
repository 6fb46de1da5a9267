"""TEST-ONLY scene builders that put particles AT the branch points of the step's wall and pair functions: tests/test_branch_point_scenes.py
proves on the CPU what every scene holds and that the oracle stays inside its bars on it, tests/test_gpu_branch_points.py runs the scenes
on the device.  Nothing in the product package imports this.

Every search evaluates the kernels' own f32 expressions in numpy float32, one rounding per operation:
  wall distance   d  = ((n_x x + n_y y) + delta) / (h_i * 2)                 OpDensity::begin / boundary_winchenbach2020.rs:68-73
  neighbour       dx dx + dy dy < s s,  s = ((h_i + h_j) * 0.5) * k           neighborhood_search.rs:138-147, oracle/neigh.c:134-136
  pair distance   q  = r / (2 h_ij) against the gradient's cut-off 1e-5       sph_kernels.rs:57-59"""
from __future__ import annotations

import numpy as np

from adaptive_sph_amd import scene as sc
from adaptive_sph_amd.workloads import dam_break_params
from tests.neighbour_scenes import h_of_mass
from tests.test_oracle_independent import _case

f32 = np.float32
LEFT, FLOOR = (1.0, 0.0, 2.0), (0.0, 1.0, 1.0)      # the two walls of the 4 x 2 box the scenes stand against
PENALTIES = ("None", "Linear", "Quadratic1", "Quadratic2")
Q_CUTOFF = 1.0e-5          # the reference zeroes grad W at q <= 1e-5
Q_FAST_ZERO = 3.0e-8       # below it the FAST pair arithmetic gives a zero gradient by itself (u^2 rounds to 4 t^2)
NLOFF_SLOTS = 24


def below(x):
    return np.nextafter(f32(x), f32(-np.inf))


def above(x):
    return np.nextafter(f32(x), f32(np.inf))


def steps_around(x, k):
    """the 2 k + 1 representable f32 values around x, ascending"""
    lo, hi = [f32(x)], [f32(x)]
    for _ in range(k):
        lo.append(below(lo[-1]))
        hi.append(above(hi[-1]))
    return np.array(lo[:0:-1] + hi, f32)


def wall_d(pos, h, plane):
    """d of every particle against one plane, in f32 as the kernel and the oracle evaluate it"""
    nx, ny, delta = (f32(v) for v in plane)
    pos, h = np.asarray(pos, f32), np.asarray(h, f32)
    return ((nx * pos[..., 0] + ny * pos[..., 1]) + delta) / (h * f32(2.0))


def tuned_mass(m0, grid=2.0 ** -20):
    """the f32 mass nearest to m0 whose support 2 h is a whole multiple of `grid`.  Behind the walls at x = -2 and y = -1 the plane
    distance x + 2 is a multiple of 2^-22, so d = sdf / (2 h) hits -1 or -0.5 EXACTLY only where 2 h (or h) lies on that lattice: one
    mass in a few hundred ulps does, 3e-5 of the mass away at most.  2^-20 leaves the same room for particles of a quarter of the mass
    (exactly half the support)."""
    bits = np.array([m0], f32).view(np.int32)[0] + np.arange(-6000, 6001)
    m = bits.astype(np.int32).view(f32)
    sr = h_of_mass(m) * f32(2.0)
    ok = np.nonzero(np.mod(sr.astype(np.float64) / grid, 1.0) == 0.0)[0]
    assert len(ok), "no such mass within 6000 ulps"
    return m[ok[np.argmin(np.abs(ok - 6000))]]


def flow(pos):
    """_case's velocity field"""
    return np.stack([0.3 * pos[:, 0] + 0.1 * pos[:, 1], -0.2 * pos[:, 1] + 0.05 * np.sin(9.0 * pos[:, 0])], 1).astype(f32)


def case_params(max_iters=3, solver="HybridDFSPH", **kw):
    """_case's parameters: forced iteration counts, max_dt 1e-4, no level estimation unless asked for"""
    return _case(max_iters, solver, **kw)[4]


# ------------------------------------------------------------------------------------------------------------------------------
# 1. wall distances
# ------------------------------------------------------------------------------------------------------------------------------
WALL_SHIFT = (-0.15, -0.07)
HAND_D = ("-1-", "-1", "-1+", "-0.5-", "-0.5", "-0.5+", "0-", "0", "0+", "1-", "1")


def _x_for_d(target, sr):
    """the x whose f32 d against the left wall is exactly `target`, found by walking the coordinate around -2 + target * sr"""
    xs = steps_around(f32(-2.0 + float(target) * float(sr)), 200)
    d = wall_d(np.stack([xs, np.zeros_like(xs)], 1), np.full(len(xs), sr / f32(2.0), f32), LEFT)
    hit = np.nonzero(d == f32(target))[0]
    assert len(hit), (target, sr)
    return xs[hit[len(hit) // 2]]


def wall_depths(handler="AnalyticOverestimate", two_sizes=False):
    """_case's jittered block (12 % denser than rest, one spacing off the left wall and the floor) moved by (-0.15, -0.07): it straddles
    both walls, with columns at d <= -1, in (-1, 0] and in (0, 1) on the left wall, rows down to d = -0.64 on the floor and a corner region
    behind both.  Above it stands a second patch of the same lattice across the left wall, and in eleven of its rows the particle nearest
    to the wanted depth is put ON it: d = -1, -0.5 and 0 exactly with the representable x on either side of each, the smallest d >= 1
    (no wall term) and the x below it (the largest d < 1 a particle of this size can have there: the last cell of the lambda table).
    The masses are tuned_mass of the block's, so those depths exist; `two_sizes`: _case's second block of a quarter of the mass stands
    on (and behind) the floor to the right.
    -> dict(scn, pos, mass, vel, planes (for ffi.Context, of `handler`), box (the four planes as tuples), hand {name: index})"""
    scn, pos, mass, vel, _ = _case(0, wall=True, two_sizes=two_sizes)
    coarse = mass == mass[0]
    m_star = tuned_mass(mass[0])
    mass = np.where(coarse, m_star, m_star * f32(0.25)).astype(f32)
    pos = (pos + np.array(WALL_SHIFT, f32)).astype(f32)
    sr = h_of_mass(m_star) * f32(2.0)
    # the patch: 8 columns x 13 rows at the block's spacing and jitter
    rng = np.random.default_rng(11)
    cx, cy = np.meshgrid(np.arange(8), np.arange(13), indexing="ij")
    patch = np.stack([-2.105 + 0.03 * cx.reshape(-1), -0.32 + 0.03 * cy.reshape(-1)], 1)
    patch = (patch + rng.uniform(-0.12, 0.12, patch.shape) * 0.03).astype(f32)
    row = cy.reshape(-1)
    wanted = {}
    for name, t in (("-1", -1.0), ("-0.5", -0.5), ("0", 0.0), ("1", 1.0)):
        x = _x_for_d(t, sr)
        wanted[name] = x
        wanted[name + "-"] = below(x)
        if name != "1":
            wanted[name + "+"] = above(x)
    hand = {}
    for k, name in enumerate(HAND_D):
        cand = np.nonzero(row == k + 1)[0]
        j = cand[np.argmin(np.abs(patch[cand, 0] - wanted[name]))]
        patch[j, 0] = wanted[name]
        hand[name] = len(pos) + int(j)
    pos = np.concatenate([pos, patch]).astype(f32)
    mass = np.concatenate([mass, np.full(len(patch), m_star, f32)])
    vel = np.concatenate([vel, flow(patch)]).astype(f32)
    box = sc.boundary_planes(scn.boundary)
    return dict(scn=scn, pos=pos, mass=mass, vel=vel, planes=sc.boundary_planes(scn.boundary, handler), box=box, hand=hand)


def wall_populations(s):
    """what wall_depths must hold, counted with the f32 d: the three intervals on the left wall, the particles behind two walls, the
    hand-placed values"""
    h = h_of_mass(s["mass"])
    dl, df = wall_d(s["pos"], h, LEFT), wall_d(s["pos"], h, FLOOR)
    return dict(deep=int((dl <= -1).sum()), behind=int(((dl > -1) & (dl <= 0)).sum()), front=int(((dl > 0) & (dl < 1)).sum()),
                floor_behind=int((df <= 0).sum()), floor_min=float(df.min()), corner=int(((dl <= 0) & (df <= 0)).sum()),
                hand={k: dl[i] for k, i in s["hand"].items()})


# ------------------------------------------------------------------------------------------------------------------------------
# 2. close pairs
# ------------------------------------------------------------------------------------------------------------------------------
# group -> the q windows its partners are placed in, one partner each (q = r / (h_i + h_j) from the f32 positions)
CLOSE_GROUPS = {
    "tiny": [(1.0e-9, 2.9e-8)] * 12,                                              # FAST: d = 4 t^2 - u^2 rounds to 0
    "band": [(1.0e-7, 1.5e-7), (2.0e-7, 4.0e-7), (0.8e-6, 1.2e-6), (2.0e-6, 3.0e-6), (6.5e-6, 7.5e-6), (9.7e-6, 9.9e-6)]
            + [(4.8e-6, 5.2e-6)] * 4 + [(8.8e-6, 9.2e-6)] * 4,                    # FAST differs from the reference
    "above": [(1.01e-5, 1.2e-5)] * 12,                                            # just past the cut-off: everybody agrees again
    "far": [(0.9e-3, 1.1e-3)] * 12,
}


def pair_q(pos, mass, i, j):
    """q of the pairs (i, j) from the f32 positions: the coordinate differences in f32 (as every kernel forms them), the rest in f64"""
    pos = np.asarray(pos, f32)
    d = (pos[i] - pos[j]).astype(np.float64)
    h = h_of_mass(mass).astype(np.float64)
    return np.sqrt((d ** 2).sum(-1)) / (h[i] + h[j])


def close_pairs(two_sizes=False):
    """_case's free block with partners appended to randomly chosen particles: 12 at r = 0 exactly, the groups of CLOSE_GROUPS, and two
    triples (two partners on one host's position).  A partner has its host's mass -- with `two_sizes` every third one the mass of the
    other size -- and its host's velocity plus a random 0.05: a pair whose gradient the reference zeroes still differs in what it would
    exchange.  Partners closer than an ulp of |x| = 0.3 stand beside hosts near an axis and are moved along the other coordinate only.
    -> dict(scn, pos, mass, vel, pairs: (host, partner, group) rows with group in zero / tiny / band / above / far)"""
    scn, pos, mass, vel, _ = _case(0, two_sizes=two_sizes)
    n0 = len(mass)
    rng = np.random.default_rng(23)
    masses = np.unique(mass)
    h_of = {float(m): float(h_of_mass(m)) for m in masses}
    used = np.zeros(n0, bool)
    new_pos, new_mass, new_vel, pairs = [], [], [], []

    def partner_mass(host):
        if two_sizes and len(pairs) % 3 == 2:
            return masses[masses != mass[host]][0]
        return mass[host]

    def add(host, p, m, group):
        used[host] = True
        pairs.append((int(host), n0 + len(new_pos), group))
        new_pos.append(np.asarray(p, f32))
        new_mass.append(f32(m))
        new_vel.append((vel[host] + rng.normal(0.0, 0.05, 2)).astype(f32))

    for _ in range(12):
        host = rng.choice(np.nonzero(~used)[0])
        add(host, pos[host], partner_mass(host), "zero")
    for _ in range(2):
        host = rng.choice(np.nonzero(~used)[0])
        add(host, pos[host], mass[host], "zero")
        add(host, pos[host], mass[host], "zero")
    for group, windows in CLOSE_GROUPS.items():
        for (lo, hi) in windows:
            for attempt in range(4000):
                fine = hi < 2.0e-6          # r below an ulp of most coordinates: hosts with a small coordinate, moved along it
                axis = int(rng.integers(0, 2))
                free = ~used & (np.abs(pos[:, axis]) < 0.0039) if fine else ~used
                host = rng.choice(np.nonzero(free)[0])
                m = partner_mass(host)
                r = np.exp(rng.uniform(np.log(lo), np.log(hi))) * (h_of[float(mass[host])] + h_of[float(m)])
                if fine:
                    step = np.zeros(2)
                    step[axis] = r * rng.choice([-1.0, 1.0])
                else:
                    th = rng.uniform(0.0, 2.0 * np.pi)
                    step = r * np.array([np.cos(th), np.sin(th)])
                p = (pos[host].astype(np.float64) + step).astype(f32)
                d = (p - pos[host]).astype(np.float64)
                q = np.sqrt((d ** 2).sum()) / (h_of[float(mass[host])] + h_of[float(m)])
                if lo <= q <= hi:
                    add(host, p, m, group)
                    break
            else:
                raise AssertionError((group, lo, hi))
    return dict(scn=scn, pos=np.concatenate([pos, np.array(new_pos, f32)]).astype(f32), mass=np.concatenate([mass, np.array(new_mass, f32)]),
                vel=np.concatenate([vel, np.array(new_vel, f32)]).astype(f32), pairs=pairs, planes=sc.boundary_planes(scn.boundary))


def close_partners(s):
    """per particle the q of its closest OTHER particle (inf without one inside 2e-3): which particles the cut-off can concern"""
    n = len(s["mass"])
    q = np.full(n, np.inf)
    for i, j, _ in s["pairs"]:
        for a, b in ((i, j), (j, i)):
            q[a] = min(q[a], float(pair_q(s["pos"], s["mass"], a, b)))
    # (the two partners of a triple are a close pair of their own)
    by_host = {}
    for i, j, _ in s["pairs"]:
        by_host.setdefault(i, []).append(j)
    for js in by_host.values():
        for a in js:
            for b in js:
                if a != b:
                    q[a] = min(q[a], float(pair_q(s["pos"], s["mass"], a, b)))
    return q


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the edge of the support
# ------------------------------------------------------------------------------------------------------------------------------
EDGE_KINDS = ("equal", "below", "above", "contracted")


def k_extended(P=None):
    """level_estimation_range / 1.9 in f32, as the step forms it (simulation.rs:2036)"""
    P = P or dam_break_params()
    return f32(P.level_estimation_range) / f32(1.9)


def predicate_terms(pos, mass, i, j, k):
    """(r2, s2) of the pairs (i, j) in f32, one rounding per operation"""
    pos, h = np.asarray(pos, f32), h_of_mass(mass)
    dx, dy = pos[i, 0] - pos[j, 0], pos[i, 1] - pos[j, 1]
    s = ((h[i] + h[j]) * f32(0.5)) * f32(k)
    return dx * dx + dy * dy, s * s


def contracted_r2(dx, dy):
    """(fma(dx, dx, dy * dy), fma(dy, dy, dx * dx)) in f32: the two forms a compiler may contract dx * dx + dy * dy into -- the exact
    product (48 bits, exact in f64) plus the rounded one, rounded once"""
    dx, dy = np.asarray(dx, f32), np.asarray(dy, f32)
    x64, y64 = dx.astype(np.float64), dy.astype(np.float64)
    return (x64 * x64 + (dy * dy).astype(np.float64)).astype(f32), (y64 * y64 + (dx * dx).astype(np.float64)).astype(f32)


def f32_neighbour_sets(pos, mass, k):
    """the neighbour sets by brute force with the f32 predicate: n x n bool"""
    pos, h = np.asarray(pos, f32), h_of_mass(mass)
    dx, dy = pos[:, None, 0] - pos[None, :, 0], pos[:, None, 1] - pos[None, :, 1]
    s = ((h[:, None] + h[None, :]) * f32(0.5)) * f32(k)
    r2 = dx * dx + dy * dy
    assert r2.dtype == f32 and s.dtype == f32
    return r2 < s * s


def _scan_edge(xi, p0, hsum_half, k, kind, span=64):
    """the representable position within +-`span` steps per coordinate of p0 whose r2 against the host xi is what `kind` asks for, the
    nearest to p0 -- or None"""
    X, Y = steps_around(p0[0], span), steps_around(p0[1], span)
    dx, dy = (xi[0] - X)[:, None], (xi[1] - Y)[None, :]
    r2 = dx * dx + dy * dy
    s = hsum_half * f32(k)
    s2 = s * s
    if kind == "equal":
        ok = r2 == s2
    elif kind == "below":
        ok = r2 == below(s2)
    elif kind == "above":
        ok = r2 == above(s2)
    else:   # the contracted form fma(dx, dx, dy dy) decides otherwise; where there is a choice, the other form fma(dy, dy, dx dx) as well
        ca, cb = contracted_r2(np.broadcast_to(dx, r2.shape), np.broadcast_to(dy, r2.shape))
        ok = (ca < s2) != (r2 < s2)
        if (ok & ((cb < s2) != (r2 < s2))).any():
            ok &= (cb < s2) != (r2 < s2)
    hit = np.argwhere(ok)
    if not len(hit):
        return None
    a, b = hit[np.argmin(np.abs(hit - span).max(axis=1))]
    return np.array([X[a], Y[b]], f32)


def support_edge(k=2.0, two_sizes=False, clumps=False, per_kind=4):
    """_case's free block moved by half a spacing, so that four particles stand within 0.02 of the origin: the hosts.  For every host and
    kind in turn a particle near the circle of radius s = h_ij k around it is moved ONTO the circle -- to the representable position whose
    f32 r2 equals s2 (not a neighbour), the value below s2 (a neighbour), the value above it, or for which dx dx + dy dy < s2 and its
    contracted forms decide differently.  `two_sizes`: every other partner gets a quarter of the mass, h_ij = (h_i + h_j) / 2.
    `clumps`: six groups of three far from the block (host A, C beside it, B on the circle around A): A's list of range k holds two or
    three entries with the edge pair -- the level estimation's `fewer than 3 entries` flag is the pair's predicate.
    -> dict(scn, pos, mass, vel, planes, k, pairs: (host, partner, kind), clumps: (A, B, C, kind))"""
    scn, pos, mass, vel, _ = _case(0)
    pos = (pos + f32(0.015)).astype(f32)
    vel = flow(pos)
    hosts = np.nonzero((np.abs(pos) < 0.02).all(axis=1))[0]
    assert len(hosts) == 4
    h = h_of_mass(mass)
    taken = np.zeros(len(mass), bool)
    taken[hosts] = True
    pairs = []
    wanted = [kind for kind in EDGE_KINDS for _ in range(per_kind if kind != "contracted" else 2 * per_kind)]
    for t, kind in enumerate(wanted):
        i = hosts[t % 4]
        m_j = mass[0] * f32(0.25) if two_sizes and t % 2 else mass[0]
        half = (h[i] + h_of_mass(m_j)) * f32(0.5)
        s = float(half * f32(k))
        d = pos.astype(np.float64) - pos[i].astype(np.float64)
        r = np.sqrt((d ** 2).sum(1))
        for j in np.argsort(np.abs(r - s)):
            if taken[j] or abs(r[j] - s) > 0.02:
                continue
            p = _scan_edge(pos[i], (pos[i].astype(np.float64) + d[j] * (s / r[j])).astype(f32), half, k, kind)
            if p is not None:
                pos[j], mass[j], taken[j] = p, m_j, True
                pairs.append((int(i), int(j), kind))
                break
        else:
            raise AssertionError((t, kind))
    out_clumps = []
    if clumps:
        extra_p, extra_m = [], []
        for c, kind in enumerate(("equal", "below", "above") * 2):
            a = np.array([-0.75 + 0.3 * c, 0.62], f32)
            m_b = mass[0] * f32(0.25) if two_sizes and c % 2 else mass[0]
            half = (h[0] + h_of_mass(m_b)) * f32(0.5)
            th = 0.4 + 0.9 * c
            u = np.array([np.cos(th), np.sin(th)])
            b = _scan_edge(a, (a.astype(np.float64) + float(half * f32(k)) * u).astype(f32), half, k, kind)
            assert b is not None, (c, kind)
            cc = (a.astype(np.float64) + 0.013 * u).astype(f32)
            base = len(mass) + len(extra_p)
            out_clumps.append((base, base + 1, base + 2, kind))
            extra_p += [a, b, cc]
            extra_m += [mass[0], m_b, mass[0]]
        pos = np.concatenate([pos, np.array(extra_p, f32)]).astype(f32)
        mass = np.concatenate([mass, np.array(extra_m, f32)]).astype(f32)
        vel = np.concatenate([vel, np.zeros((len(extra_p), 2), f32)])
    return dict(scn=scn, pos=pos, mass=mass, vel=vel, planes=sc.boundary_planes(scn.boundary), k=f32(k), pairs=pairs, clumps=out_clumps)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. a gentle uniform scene for the record and offset forms: many steps
# ------------------------------------------------------------------------------------------------------------------------------
def wall_records(nx=32, ny=32, spacing=1.0 / 32):
    """dam_break_small (fill 0.93, at rest spacing) moved 1.5 spacings to the left: its first column stands behind the left wall
    (d = -0.23: wall terms from step 0 on the side the penalties act on), the floor one spacing below it as before.  A 3 x 3 patch in the
    interior is tripled -- exact duplicates, as scene blocks on a common lattice give them: the list of its middle holds 30 others, more
    than an offset list.  Duplicates never part (no gradient between them, equal velocities), so the patch stays three times too dense
    and throws its surroundings apart: the steps run without an error, but this is no scene to compare two arithmetics on."""
    scn = sc.dam_break_small(nx, ny, spacing)
    pos, mass, vel = sc.init_particles(scn)
    pos = pos.copy()
    pos[:, 0] = (pos[:, 0] - f32(1.5 * spacing)).astype(f32)
    ix, iy = np.arange(len(mass)) // ny, np.arange(len(mass)) % ny
    patch = np.nonzero((np.abs(ix - 20) <= 1) & (np.abs(iy - 12) <= 1))[0]
    extra = np.concatenate([patch, patch])
    return dict(scn=scn, pos=np.concatenate([pos, pos[extra]]).astype(f32), mass=np.concatenate([mass, mass[extra]]),
                vel=np.concatenate([vel, vel[extra]]).astype(f32), planes=sc.boundary_planes(scn.boundary), centre=int(patch[len(patch) // 2]))


RECORD_STEPS = 12


def wall_records_params(**kw):
    """three forced iterations per solve: the tripled patch keeps the free-running loops at their cap"""
    return dam_break_params(max_dt=2.0e-4, max_iters=3, hybrid_dfsph_max_avg_density_error=0.0, hybrid_dfsph_max_avg_divergence_error=0.0,
                            iisph_max_avg_density_error=0.0, **kw)
