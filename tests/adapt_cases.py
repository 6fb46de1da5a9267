"""Designed inputs for the apply half of single_step_adaptivity (share_particles / merge_particles / split_particles) and the three
sequential float32 models written from the reference's text (adaptivity/particle_sharing.rs:152-253, particle_merging.rs:270-385,
splitting.rs:19-82).  numpy only: tests/test_adapt_cases.py checks every case against the CPU oracle and that it still hits the branch
it is named after, tests/test_gpu_adapt_branch_points.py runs the same cases on the device.

A case is a `Case`: (n, mass, position, velocity, h2, h2_next, level, level_old, size_class, merge_partner, merge_counter, overrides) and
what the tests need beside the arrays (kind, dt, capacity, the expected status of a designed refusal).  Every per-particle field holds a
distinct value per particle and level_old = arange(n) is the identity tag, so a regather that moves one field with the wrong particle
shows.  The particles sit on a lattice inside the 4 x 2 box with a donor and its receivers on neighbouring sites: the state an apply
leaves behind can be stepped."""
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

from adaptive_sph_amd import adaptivity as A, ffi
from adaptive_sph_amd.workloads import dam_break_params

f32 = np.float32
AV, DEL = ffi.MERGE_PARTNER_AVAILABLE, ffi.MERGE_PARTNER_DELETE
TOO_LARGE = 4
REPO = Path(__file__).resolve().parent.parent
PATTERNS = REPO / "tests" / "golden" / "split-patterns.yaml"
S = 1.0 / 64                       # lattice spacing
M0 = f32(0.93) * f32(S) * f32(S)   # mass of a lattice particle (dam_break_small's fill ratio)
SCAN_TILE, SCAN_BLOCK = 2048, 256  # device_exclusive_scan_u32 (sph_adapt.hip)
FIELDS = ("mass", "position", "velocity", "h2", "h2_next", "level_estimation", "level_old", "particle_size_class")   # what sph_upload_field takes


# ---- the sequential models ------------------------------------------------------------------------------------------------------
def h_from_mass(m, rho0):
    """FluidSimulation::h_from_mass (simulation.rs:371-380): ETA * sphere_volume_to_radius(mass / rest_density)"""
    return f32(1.9) * np.sqrt((f32(m) / f32(rho0)) * f32(1 / np.pi), dtype=np.float32)


def merge_model(mass, pos, vel, h2n, partner, counter, min_partners, rho0):
    """particle_merging.rs:270-370 on python lists of per-particle records (everything swaps together)."""
    f32 = np.float32
    n = len(mass)
    mass, pos, vel, h2n = mass.copy(), pos.copy(), vel.copy(), h2n.copy()
    ident = np.arange(n)
    partner, counter = partner.copy(), counter.copy()
    m0, x0, v0 = mass.copy(), pos.copy(), vel.copy()
    for i in range(n):
        j = partner[i]
        if j in (AV, DEL) or counter[j] < min_partners:
            continue
        mass_n = f32(m0[j]) / f32(counter[j])
        m = f32(m0[i]) + mass_n
        vel[i] = (f32(m0[i]) * v0[i] + mass_n * v0[j]) / m
        pos[i] = (f32(m0[i]) * x0[i] + mass_n * x0[j]) / m
        mass[i] = m
        h2n[i] = f32(1.9) * np.sqrt((m / f32(rho0)) * f32(1 / np.pi), dtype=np.float32)
    last, i = n - 1, 0
    while i <= last:
        if partner[i] == DEL and counter[i] >= min_partners:
            mass[i] = mass[i] - mass[i]
            if mass[i] < 0.000001:
                for a in (mass, pos, vel, h2n, ident, partner, counter):
                    a[[i, last]] = a[[last, i]]
                last -= 1
                continue
        i += 1
    k = last + 1
    return mass[:k], pos[:k], vel[:k], h2n[:k], ident[:k]


def dropped_mass_sharing(mass, target, max_transfer, dt):
    """particle_sharing.rs:242-253 -> (dropped mass, which arm of the min it is: 0 = mass - target, 1 = target * max_transfer * dt)"""
    a, b = f32(mass) - f32(target), f32(target) * f32(max_transfer) * f32(dt)
    return (a, 0) if a < b else (b, 1)


def share_model(mass, pos, vel, h2n, level, partner, counter, min_partners, P, dt):
    """particle_sharing.rs:152-240: the receivers read their donors as they were before the call, then the donors drop their mass.
    -> mass, position, velocity, h2_next and, per donor that gave, the arm of the min."""
    n = len(mass)
    target = A.target_mass(np.asarray(level, np.float32), P)
    m0, x0, v0 = mass.copy(), pos.copy(), vel.copy()
    mass, pos, vel, h2n = mass.copy(), pos.copy(), vel.copy(), h2n.copy()
    arms = {}
    for i in range(n):
        j = int(partner[i])
        if j in (AV, DEL) or counter[j] < min_partners:
            continue
        dropped, _ = dropped_mass_sharing(m0[j], target[j], P.max_mass_transfer_sharing, dt)
        mass_n = dropped / f32(counter[j])
        m = f32(m0[i]) + mass_n
        vel[i] = (f32(m0[i]) * v0[i] + mass_n * v0[j]) / m
        pos[i] = (f32(m0[i]) * x0[i] + mass_n * x0[j]) / m
        mass[i] = m
        h2n[i] = h_from_mass(m, P.rest_density)
    for i in range(n):
        if partner[i] != DEL or counter[i] < min_partners:
            continue
        dropped, arms[i] = dropped_mass_sharing(m0[i], target[i], P.max_mass_transfer_sharing, dt)
        mass[i] = f32(m0[i]) - dropped
        h2n[i] = h_from_mass(mass[i], P.rest_density)
    return mass, pos, vel, h2n, arms


def round_half_away(q):
    """f32::round for q >= 0 (numpy's round goes to even)"""
    t = np.floor(f32(q))
    return t + f32(1) if f32(q) - t >= f32(0.5) else t


def num_children(mass, target, max_children, fail_on_missing):
    """splitting.rs:28-44 -> the child count, or None where the reference panics"""
    r = round_half_away(f32(mass) / f32(target))
    nc = int(r) if r > 0 else 0
    if nc > max_children:
        if fail_on_missing:
            return None
        nc = max_children
    return nc if nc > 1 else None


def split_model(c, patterns, capacity):
    """splitting.rs:19-82 on the fields of a case -> (status, fields): the children are appended in the order of their parents' indices,
    h2 and level_old of an appended child stay at ParticleVec's defaults (the reference writes them to the parent's slot, :73, :76)."""
    P = c.params()
    rho0 = f32(P.rest_density)
    max_children = len(patterns) + 1
    target = A.target_mass(c.level, P)
    out = {"mass": list(c.mass), "position": [x.copy() for x in c.position], "velocity": [v.copy() for v in c.velocity], "h2": list(c.h2),
           "h2_next": list(c.h2_next), "level_estimation": list(c.level), "level_old": list(c.level_old), "particle_size_class": list(c.size_class)}
    for i in range(c.n):
        if c.size_class[i] != TOO_LARGE:
            continue
        if np.isnan(c.level[i]):
            return 27, None
        nc = num_children(c.mass[i], target[i], max_children, P.fail_on_missing_split_pattern)
        if nc is None:
            return 27, None
        if len(out["mass"]) + nc - 1 > capacity:
            return 3, None
        pat = patterns[nc - 2]
        radius = np.sqrt((f32(c.mass[i]) / f32(1.0)) * f32(1 / np.pi), dtype=np.float32)
        cm = f32(c.mass[i]) / f32(nc)
        hn = h_from_mass(cm, rho0)
        out["mass"][i], out["position"][i], out["h2"][i], out["h2_next"][i] = cm, c.position[i] + pat[0] * radius, hn, hn
        for k in range(1, nc):
            for name, v in (("mass", cm), ("position", c.position[i] + pat[k] * radius), ("velocity", c.velocity[i].copy()), ("h2", f32(0)), ("h2_next", hn),
                            ("level_estimation", c.level[i]), ("level_old", f32(0)), ("particle_size_class", np.uint8(2))):
                out[name].append(v)
    return 0, {k: np.asarray(v, dtype=ffi.FIELDS[k][1]) for k, v in out.items()}


# ---- a case -----------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    n: int
    mass: np.ndarray
    position: np.ndarray
    velocity: np.ndarray
    h2: np.ndarray
    h2_next: np.ndarray
    level: np.ndarray
    level_old: np.ndarray
    size_class: np.ndarray
    merge_partner: np.ndarray
    merge_counter: np.ndarray
    overrides: dict = field(default_factory=dict)      # SimulationParams fields (the adapt parameters among them)
    kind: str = "merge"
    name: str = ""
    dt: float = 0.001
    capacity: int = 0                                  # of the contexts the case is uploaded to
    patterns: bool = True                              # split: whether the pattern table is set
    status: int = 0                                    # 0, or the status of the designed refusal
    note: dict = field(default_factory=dict)           # what the builder designed: checked by test_adapt_cases.py

    def params(self):
        return dam_break_params(level_estimation_method="None", **self.overrides)

    def adapt_params(self):
        return A.adapt_params(self.params(), self.dt)

    def fields(self):
        return {"mass": self.mass, "position": self.position, "velocity": self.velocity, "h2": self.h2, "h2_next": self.h2_next,
                "level_estimation": self.level, "level_old": self.level_old, "particle_size_class": self.size_class}


def lattice(n, groups=(), spacing=S):
    """positions of n particles on a lattice inside the box, the members of every group (a donor and its receivers) on consecutive sites"""
    width = 64 if n <= 8192 else 1024
    order, seen = [], np.zeros(n, bool)
    for g in groups:
        for i in g:
            if not seen[i]:
                seen[i] = True
                order.append(i)
    order = np.concatenate([np.asarray(order, np.int64), np.nonzero(~seen)[0]])
    site = np.empty(n, np.int64)
    site[order] = np.arange(n)
    s = f32(spacing)
    x = f32(-2.0) + f32(1.024) * s + (site % width).astype(np.float32) * s
    y = f32(-1.0) + f32(1.024) * s + (site // width).astype(np.float32) * s
    return np.stack([x, y], axis=1).astype(np.float32)


def base_case(n, groups=(), spacing=S, m0=None, **kw):
    """n lattice particles, every field distinct per particle (exactly: i * 2^-20 is a float32 step for i < 2^20)"""
    i = np.arange(n, dtype=np.float64)
    m0 = f32(M0 if m0 is None else m0) * (f32(spacing) / f32(S)) ** 2
    mass = (np.float64(m0) * (1.0 + i * 2.0 ** -20)).astype(np.float32)
    velocity = np.stack([i * 2.0 ** -20 - 0.25, 0.125 - i * 2.0 ** -21], axis=1).astype(np.float32)
    h2_next = h_from_mass(mass, 1.0).astype(np.float32)
    h2 = (h2_next * f32(1 + 2.0 ** -10)).astype(np.float32)
    level = (-(i + 1.0) * 2.0 ** -21).astype(np.float32)
    c = Case(n, mass, lattice(n, groups, spacing), velocity, h2, h2_next, level, np.arange(n, dtype=np.float32), (np.arange(n) % 4).astype(np.uint8),
             np.full(n, AV, np.uint32), np.zeros(n, np.uint16), **kw)
    c.capacity = c.capacity or n + 64
    assert len(np.unique(mass)) == n and len(np.unique(velocity[:, 0])) == n and len(np.unique(c.position, axis=0)) == n and len(np.unique(level)) == n
    return c


def decide(c, groups):
    """groups: [donor, receiver, ...]"""
    for g in groups:
        d, recv = g[0], g[1:]
        assert c.merge_partner[d] == AV and all(c.merge_partner[r] == AV for r in recv) and d not in recv
        c.merge_partner[d] = DEL
        c.merge_partner[list(recv)] = d
        c.merge_counter[d] = len(recv)
    return c


# ---- merge: where the closed-form deletion could differ from the swap-with-the-last loop --------------------------------------
def groups_for(n, donors, n_recv=lambda k: 1 + k % 3, exclude=()):
    """every donor with n_recv(k) receivers taken in ascending order from the particles that are neither donors nor excluded"""
    taken = np.zeros(n, bool)
    taken[list(donors)] = True
    taken[list(exclude)] = True
    free = iter(np.nonzero(~taken)[0].tolist())
    out = []
    for k, d in enumerate(donors):
        recv = []
        for _ in range(n_recv(k)):
            r = next(free, None)
            if r is not None:
                recv.append(r)
        out.append([int(d)] + recv)
    return out


def merge_case(name, n, groups, min_partners=0, **kw):
    c = decide(base_case(n, groups, kind="merge", name=name, overrides={"minimum_merge_partners": min_partners}, **kw), groups)
    del_ = (c.merge_partner == DEL) & (c.merge_counter >= min_partners)
    c.note.update(n_del=int(del_.sum()), n_new=int(n - del_.sum()), deleted=np.nonzero(del_)[0])
    return c


def merge_cases():
    out = []
    n = 600
    out.append(merge_case("tail only", n, groups_for(n, range(n - 40, n))))
    out.append(merge_case("head only", n, groups_for(n, range(40), exclude=range(40, 300))))
    out.append(merge_case("last k + scattered", n, groups_for(n, list(range(7, 500, 7)) + list(range(n - 17, n)))))
    n = 300
    for label, keep in (("all but one", 137), ("all but the last", n - 1), ("all but the first", 0)):
        d = (keep + 1) % n                                              # the survivor receives from one donor, everybody else just goes
        out.append(merge_case(label, n, [[d, keep]] + [[i] for i in range(n) if i not in (d, keep)]))
    out.append(merge_case("everything", 257, [[i] for i in range(257)]))
    out.append(merge_case("n = 1", 1, [[0]]))
    out.append(merge_case("n = 1, kept", 1, []))
    out.append(merge_case("n = 2", 2, [[0, 1]]))
    n = 600
    donors = list(range(n - 30, n))                                     # min_partners = 2: the donors with one receiver stay, inside the tail
    out.append(merge_case("minimum partners keeps a donor in the tail", n, groups_for(n, donors, n_recv=lambda k: 1 + k % 2), min_partners=2))
    out.append(merge_case("n_new = 256, n_del = 256", 512, groups_for(512, range(1, 512, 2), n_recv=lambda k: 1)))
    out.append(merge_case("n_new = 256, n_del = 257", 513, groups_for(513, range(0, 513, 2), n_recv=lambda k: 1 if k < 256 else 0)))
    for n, mp in ((2047, 0), (2048, 2), (2049, 0), (4096, 0), (4097, 2)):
        edges = [e for t in range(SCAN_TILE, n + 1, SCAN_TILE) for e in (t - 1, t) if e < n]       # both sides of every tile edge
        donors = sorted(set(edges) | set(range(3, n, 5)) | {0, n - 1})
        # min_partners = 2: one receiver at the donors left of an edge and at every sixth (they stay), two or three elsewhere
        nr = (lambda k: 1 + k % 3) if mp == 0 else (lambda k, donors=donors: 1 if (donors[k] + 1) % SCAN_TILE == 0 or k % 6 == 0 else 2 + k % 2)
        donors = donors[: n // 4] if mp else donors
        out.append(merge_case(f"n = {n}, minimum_merge_partners = {mp}", n, groups_for(n, donors, n_recv=nr), min_partners=mp))
    return out


def merge_case_large():
    """n = 524 289: the scan of the block sums walks a second chunk (more than 256 tiles)"""
    n = 256 * SCAN_TILE + 1
    donors = [5] + list(range(SCAN_TILE, n - SCAN_TILE, 3)) + [n - 1]                # (the last tile holds one particle: n - 1)
    groups = [[5, 6]] + [[d, d + 1] for d in donors[1:-1]] + [[n - 1, n - 2]]
    return merge_case("n = 524289", n, groups, spacing=1.0 / 1024, capacity=600000)


# ---- share: both arms of the min, the clamp of the level, minimum_share_partners ------------------------------------------------
MSD = 0.5   # maximum_surface_distance of the share and split cases


def sizing_overrides(sizing, fine_mass):
    """radii that put target_mass(level 0) at fine_mass and target_mass(level <= -MSD) at four times that"""
    r_fine = float(np.sqrt(np.float64(fine_mass) / np.pi))
    return {"sizing_function": sizing, "particle_radius_fine": r_fine, "particle_radius_base": 2 * r_fine, "maximum_surface_distance": MSD, "rest_density": 1.0}


def share_case(sizing, min_partners, n=700):
    donors = list(range(2, n - 200, 9)) + [n - 1]
    groups = groups_for(n, donors, n_recv=lambda k: 1 + k % 3)
    ov = dict(sizing_overrides(sizing, M0 / f32(4)), minimum_share_partners=min_partners, max_mass_transfer_sharing=250.0)
    c = decide(base_case(n, groups, kind="share", name=f"share {sizing}, minimum_share_partners = {min_partners}", overrides=ov, dt=0.001), groups)
    P = c.params()
    assert P.max_mass_transfer_sharing * c.dt < 1
    levels = [0.0, -MSD / 2, -MSD, -2 * MSD]
    for k, d in enumerate(donors):
        c.level[d] = f32(levels[k % 4] if k % 4 != 1 else levels[1] * (1 + (k // 4) * 2.0 ** -12))
    target = A.target_mass(c.level, P)
    for k, d in enumerate(donors):
        # first arm: a little above the target; second arm: twice the target (the transfer is capped at target * max_transfer * dt)
        c.mass[d] = target[d] * (f32(1 + 2.0 ** -10) + f32(k * 2.0 ** -20)) if (k // 4) % 2 == 0 else target[d] * (f32(2) + f32(k * 2.0 ** -19))
        c.size_class[d] = 3
    c.h2_next = h_from_mass(c.mass, 1.0).astype(np.float32)
    c.note.update(donors=donors, levels=levels)
    return c


def share_cases():
    return [share_case("Mass", 0), share_case("Radius", 2), share_case("Radius", 0, n=2049)]


# ---- split: ties of round(m / target), the clamp to the table, refusals, plateaus of the prefix sum, capacity ------------------
def tie_mass(target, ratio):
    """a mass a few ulps around target * ratio with f32(mass / target) == ratio, or None"""
    m = f32(target) * f32(ratio)
    lo = hi = m
    for _ in range(8):
        lo, hi = np.nextafter(lo, f32(0)), np.nextafter(hi, f32(np.inf))
    while lo <= hi:
        if f32(lo) / f32(target) == f32(ratio):
            return f32(lo)
        lo = np.nextafter(lo, f32(np.inf))
    return None


TIES = (1.5, 2.5, 3.5, 58.5, 59.5)
JUST_BELOW = float(np.nextafter(f32(1.5), f32(0)))   # 1.4999999


def split_case(name, sizing, n, parents, ratios, fail_on_missing=False, interp_levels=None, nan_at=None, capacity=None, patterns=True, status=0, slack=0):
    """parents[k] gets the mass with f32(mass / target) == ratios[k] (ratios cycle); levels spread over the sizing function's range"""
    fine = M0 / f32(64)
    ov = dict(sizing_overrides(sizing, fine), fail_on_missing_split_pattern=fail_on_missing)
    c = base_case(n, kind="split", name=name, overrides=ov, patterns=patterns, status=status)
    c.size_class[c.size_class == TOO_LARGE] = 2
    P = c.params()
    levels = interp_levels if interp_levels is not None else [0.0, -MSD / 4, -MSD / 2, -MSD, -2 * MSD]
    found = {}
    for k, i in enumerate(parents):
        ratio = ratios[k % len(ratios)]
        for shift in range(64):                                          # which ties exist depends on the target: walk the level until one does
            lv = f32(levels[k % len(levels)])
            lv = f32(lv * (1 + (k + 97 * shift) * 2.0 ** -14)) if interp_levels is None and lv != 0 else lv
            m = tie_mass(A.target_mass(np.asarray([lv], np.float32), P)[0], ratio)
            if m is not None or interp_levels is not None:
                break
        if m is None:
            continue
        c.level[i], c.mass[i], c.size_class[i] = lv, m, TOO_LARGE
        found.setdefault(ratio, []).append(i)
    if nan_at is not None:
        c.level[nan_at] = np.nan
    c.h2_next = h_from_mass(c.mass, 1.0).astype(np.float32)
    sp = A.SplitPatterns.load_from_file(PATTERNS)
    target = A.target_mass(c.level, P)
    kids = [num_children(c.mass[i], target[i], sp.get_max_num_children(), fail_on_missing) for i in np.nonzero(c.size_class == TOO_LARGE)[0]]
    extra = sum(k - 1 for k in kids if k)
    c.capacity = capacity if capacity is not None else n + extra + slack
    c.note.update(found=found, extra=extra, parents=np.nonzero(c.size_class == TOO_LARGE)[0])
    return c


def split_cases():
    out = []
    n = 700
    runs = [0, 1, 2, 50, 51, 300, 301, 302, 303, n - 2, n - 1] + list(range(100, 280, 13))       # indices 0 and n - 1, runs of neighbours
    for sizing in ("Mass", "Radius"):
        out.append(split_case(f"ties, {sizing}", sizing, n, runs, TIES, slack=5))
        out.append(split_case(f"59.5 refused with the flag on, {sizing}", sizing, n, runs, (2.5, 59.5), fail_on_missing=True, status=27, slack=5))
        out.append(split_case(f"1.4999999, {sizing}", sizing, n, runs, (2.5, 3.5, JUST_BELOW), status=27, slack=5))
    out.append(split_case("capacity of exactly n + extra", "Mass", n, runs, TIES))
    c = split_case("capacity one short", "Radius", n, runs, TIES, status=3)
    c.capacity -= 1
    out.append(c)
    out.append(split_case("a NaN level on a TooLarge particle", "Mass", n, runs, (2.5, 3.5), nan_at=runs[5], status=27, slack=5))
    out.append(split_case("no pattern table", "Radius", n, runs, (2.5,), patterns=False, status=27, slack=5))
    out.append(split_case("nobody splits", "Mass", 300, [], TIES, slack=5))
    out.append(split_case("n = 2049, parents on both sides of the tile edge", "Mass", 2049, [0, 2046, 2047, 2048] + list(range(5, 2040, 37)), TIES, slack=5))
    # the third sizing function only where powf is exact: interp 0 and 1
    out.append(split_case("Radius2 at interp 0 and 1", "Radius2", n, runs, TIES, interp_levels=[0.0, -MSD, -2 * MSD], slack=5))
    return out


# ---- slab cases: decisions in global ids on dam_break_small(96, 48, 1/48), chosen from the group's own neighbour lists ----------
SLAB_SPACING = 1.0 / 48


def slab_scene(interleaved=False):
    """-> (pos, mass, vel, planes): the scene test_gpu_slabs.py runs at k = 2, 3 and 4, the masses made distinct per particle.  The scene's
    own order is x-outer, so every rank owns one contiguous range of ids; interleaved: the particles in a fixed shuffled order, so that
    neighbouring ids lie on different ranks."""
    from adaptive_sph_amd import scene as sc
    scn = sc.dam_break_small(96, 48, SLAB_SPACING)
    pos, mass, vel = sc.init_particles(scn)
    if interleaved:
        perm = np.random.default_rng(7).permutation(len(mass))
        pos, vel = pos[perm], vel[perm]
    mass = (mass.astype(np.float64) * (1.0 + np.arange(len(mass)) * 2.0 ** -20)).astype(np.float32)
    return pos, mass, vel, sc.boundary_planes(scn.boundary)


def slab_rank_of(ids_per_rank, n):
    rank = np.full(n, -1, np.int64)
    for r, ids in enumerate(ids_per_rank):
        rank[np.asarray(ids, np.int64)] = r
    assert (rank >= 0).all()
    return rank


def slab_overrides(fine_mass, **kw):
    return dict(sizing_overrides("Mass", fine_mass), **kw)


def slab_pairs(n, off, idx, want, n_recv=lambda d: 1 + d % 3):
    """want(d) -> None or a predicate on the receiver: donors in ascending id, each with up to n_recv(d) receivers among its free neighbours"""
    partner, counter = np.full(n, AV, np.uint32), np.zeros(n, np.uint16)
    for d in range(n):
        if partner[d] != AV:
            continue
        ok = want(d)
        if ok is None:
            continue
        recv = [int(j) for j in idx[off[d]:off[d + 1]] if j != d and partner[j] == AV and ok(int(j))][: n_recv(d)]
        if not recv:
            continue
        partner[d], counter[d] = DEL, len(recv)
        partner[recv] = d
    return partner, counter


def slab_transfer_cases(n, rank, off, idx, mass):
    """-> [dict(name, kind, partner, counter, level, overrides, dt)] for a k-rank group in the scene's own order (rank r owns a contiguous
    range of ids): every donor is a neighbour of its receivers (the slab form reads a donor across a cut from the ghost layer)."""
    k = int(rank.max()) + 1
    out = []
    m = f32(np.median(mass))
    level0 = (-(np.arange(n) + 1.0) * 2.0 ** -21).astype(np.float32)
    # pairs that straddle each cut in both directions: a donor on rank r with receivers on r + 1 (even ids) or on r - 1 (odd ids)
    straddle = lambda d: (lambda j, w=rank[d] + (1 if d % 2 == 0 else -1): rank[j] == w)
    for mp in (0, 2):
        partner, counter = slab_pairs(n, off, idx, straddle)
        out.append(dict(name=f"straddling pairs, merge, minimum_merge_partners = {mp}", kind="merge", partner=partner, counter=counter, level=level0,
                        overrides=slab_overrides(m / f32(4), minimum_merge_partners=mp)))
    # share across the cuts, both arms of the min: level 0 puts the target at a quarter of the mass (the cap wins), a level just above
    # -MSD puts it just below the mass (mass - target wins)
    partner, counter = slab_pairs(n, off, idx, straddle)
    level = level0.copy()
    donors = np.nonzero(partner == DEL)[0]
    level[donors[1::2]] = f32(-MSD * (1 - 2.0 ** -6))
    out.append(dict(name="straddling pairs, share", kind="share", partner=partner, counter=counter, level=level,
                    overrides=slab_overrides(m / f32(4), minimum_share_partners=0, max_mass_transfer_sharing=250.0)))
    # every hole below n' on rank 0, every tail survivor on the last rank: donors on rank 0 only, fewer than the last rank owns
    partner, counter = slab_pairs(n, off, idx, lambda d: (lambda j: rank[j] == 0) if rank[d] == 0 and d % 4 == 0 else None,
                                  n_recv=lambda d: 1 + (d // 4) % 3)
    out.append(dict(name="holes on rank 0, tail survivors on the last rank", kind="merge", partner=partner, counter=counter, level=level0,
                    overrides=slab_overrides(m / f32(4), minimum_merge_partners=0)))
    # one rank whose particles are all donors (minimum_merge_partners = 0: a donor without a receiver goes as well)
    whole = 1 if k > 2 else 0
    partner, counter = slab_pairs(n, off, idx, lambda d: (lambda j: rank[j] != whole) if rank[d] == whole else None)
    partner[(rank == whole) & (partner == AV)] = DEL
    out.append(dict(name="one rank is all donors", kind="merge", partner=partner, counter=counter, level=level0, whole=whole,
                    overrides=slab_overrides(m / f32(4), minimum_merge_partners=0)))
    for c in out:
        c.setdefault("dt", 0.001)
    return out


def slab_split_cases(n, rank, pos, mass, cuts, n_parents=24):
    """-> [dict(name, parents, ratios -> mass, level, size_class, overrides)] for a k-rank group in the interleaved order: the parents alternate
    between the ranks by id, one with 59 children sits next to every cut; and the same with one rank left without parents."""
    k = int(rank.max()) + 1
    m = f32(np.median(mass))
    ov = slab_overrides(m / f32(64), fail_on_missing_split_pattern=False)
    P = dam_break_params(level_estimation_method="None", **ov)
    out = []
    for name, ranks in (("parents alternate between the ranks by id", list(range(k))), ("one rank without parents", list(range(1, k)))):
        parents, want = [], 0
        for i in range(n):                                      # ascending ids, the ranks in turn
            if rank[i] == ranks[want % len(ranks)]:
                parents.append(i)
                want += 1
                if len(parents) == n_parents:
                    break
        near = []
        for cut in cuts[1:-1]:                                   # the particle closest to each cut, among the ranks that split
            cand = np.nonzero(np.isin(rank, ranks))[0]
            near.append(int(cand[np.argmin(np.abs(pos[cand, 0] - f32(cut)))]))
        level = np.zeros(n, np.float32)
        size_class = np.full(n, 2, np.uint8)
        new_mass = mass.copy()
        t0 = A.target_mass(np.zeros(1, np.float32), P)[0]
        ratios = {}
        for q, i in enumerate(sorted(set(parents) | set(near))):
            ratio = 59.5 if i in near else TIES[q % 4]
            tm = tie_mass(t0, ratio)
            if tm is None:
                tm = f32(t0) * f32(3.25)                            # (this tie does not exist at this target: no tie, four children)
                ratio = float(tm / f32(t0))
            new_mass[i], size_class[i], ratios[i] = tm, TOO_LARGE, ratio
        out.append(dict(name=name, kind="split", parents=np.asarray(sorted(ratios)), ratios=ratios, near=near, mass=new_mass, level=level, size_class=size_class,
                        overrides=ov, dt=0.001, ranks=ranks))
    return out


def slab_case(spec, mass, position, velocity, h2, h2_next):
    """a slab spec and the fields of the stepped group, gathered by id, as a Case (ids are the reference's indices)"""
    n = len(mass)
    return Case(n, spec.get("mass", mass).astype(np.float32), position, velocity, h2, h2_next, spec["level"], np.arange(n, dtype=np.float32),
                spec.get("size_class", (np.arange(n) % 4).astype(np.uint8)), spec.get("partner", np.full(n, AV, np.uint32)), spec.get("counter", np.zeros(n, np.uint16)),
                overrides=spec["overrides"], kind=spec["kind"], name=spec["name"], dt=spec["dt"], capacity=n + 4096, note=spec)


def upload(lib, c, capacity=None):
    """a context of `lib` (the oracle or the product) holding the case: sph_upload, then every field sph_upload_field takes"""
    from adaptive_sph_amd import scene as sc
    PLANES = sc.boundary_planes(sc.dam_break_small().boundary)
    ctx = ffi.Context(lib, capacity or c.capacity, PLANES)
    ctx.upload(c.mass, c.position, c.velocity)
    for name, v in c.fields().items():
        ctx.upload_field(name, v)
    return ctx


def check_slab_transfer_case(c, rank):
    """the branch a slab transfer case is named after (also called by the GPU file on the cases it builds from the group's lists)"""
    k = int(rank.max()) + 1
    spec, partner = c.note, c.merge_partner
    recv = np.nonzero(partner < DEL)[0]
    don = partner[recv].astype(np.int64)
    mp = int(c.params().minimum_merge_partners if c.kind == "merge" else c.params().minimum_share_partners)
    deleted = np.nonzero((partner == DEL) & (c.merge_counter >= mp))[0] if c.kind == "merge" else np.zeros(0, np.int64)
    n_new = c.n - len(deleted)
    if c.name.startswith("straddling"):
        crossings = {(int(a), int(b)) for a, b in zip(rank[don], rank[recv])}
        assert crossings >= {(r, r + 1) for r in range(k - 1)} | {(r + 1, r) for r in range(k - 1)}, crossings
        assert {1, 2} <= {int(x) for x in c.merge_counter[partner == DEL]}
        if mp == 2:
            assert ((partner == DEL) & (c.merge_counter < 2)).any()
    elif c.name.startswith("holes on rank 0"):
        holes, tail = deleted[deleted < n_new], np.setdiff1d(np.arange(n_new, c.n), deleted)
        assert len(holes) > 100 and (rank[holes] == 0).all() and len(tail) == len(holes) and (rank[tail] == k - 1).all()
    elif c.name.startswith("one rank is all"):
        w = spec["whole"]
        assert np.array_equal(np.sort(deleted), np.nonzero(rank == w)[0]) and (rank[recv] != w).all() and len(recv) > 10
    return deleted


def check_slab_split_case(c, rank):
    k = int(rank.max()) + 1
    spec = c.note
    parents = spec["parents"]
    assert set(rank[parents].tolist()) == set(spec["ranks"])
    alt = [i for i in parents if i not in spec["near"]]
    assert (np.diff(rank[alt[:20]]) != 0).all() or len(spec["ranks"]) == 1                  # neighbouring parents (by id) on different ranks
    assert len(spec["near"]) == k - 1 and all(spec["ratios"][i] == 59.5 for i in spec["near"])
    if c.name.startswith("one rank without"):
        assert not (rank[parents] == 0).any() and (rank == 0).any()
