"""Host-side half of ``single_step_adaptivity`` (reference: src/simulation/simulation.rs:2732-2796).

The reference takes the share / merge partner DECISIONS in a sequential loop over the particles
(adaptivity/particle_sharing.rs:14-117, particle_merging.rs:16-125) -- that stays on the host, here as on the Rust side --
and the particle DATA stays on the device: the host reads the handful of fields the decision needs plus the neighbour lists,
fills ``merge_partner`` / ``merge_counter`` exactly as the reference does, and hands the two arrays to the library
(``sph_share_particles`` / ``sph_merge_particles`` / ``sph_split_particles``, include/sph_ffi.h), which applies them to the
device-resident state with the reference's Vec semantics.

All comparisons are made on float32 values with the reference's operation order (numpy float32 scalars).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import yaml

from . import ffi
from .simulation_parameters import SimulationParams

f32 = np.float32

# ParticleSizeClass (adaptivity/mod.rs:12-23)
TOO_SMALL, SMALL, OPTIMAL, LARGE, TOO_LARGE = 0, 1, 2, 3, 4
PARTICLE_SIZE_FACTOR_LARGE = f32(1.1)          # adaptivity/mod.rs:26
MERGE_PARTNER_AVAILABLE = ffi.MERGE_PARTNER_AVAILABLE
MERGE_PARTNER_DELETE = ffi.MERGE_PARTNER_DELETE
PI = f32(np.pi)


class SplitPatterns:
    """``SplitPatterns<2>`` (splitting.rs:84-120): entry k is the 1-to-(k+2) split, child offsets in parent radii."""

    def __init__(self, patterns: Sequence[np.ndarray]):
        for i, q in enumerate(patterns):
            if np.asarray(q).shape != (i + 2, 2):
                raise ValueError("assertion failed: sp.pos_s.len() == i + 2")
        self.patterns: List[np.ndarray] = [np.asarray(q, np.float32) for q in patterns]

    @classmethod
    def load_from_file(cls, path) -> "SplitPatterns":
        """load_split_patterns_from_file (simulation.rs:3000-3004): the serde_yaml form of Vec<SplitPattern> (mass_s, pos_s, h_s)."""
        with open(path, "r") as fh:
            doc = yaml.safe_load(fh)
        out = []
        for k, entry in enumerate(doc):
            pos = np.asarray(entry["pos_s"], np.float32)
            if len(entry["mass_s"]) != len(pos) or len(entry["h_s"]) != len(pos):
                raise ValueError(f"split pattern {k}: mass_s / pos_s / h_s lengths differ")
            out.append(pos)
        return cls(out)

    def get_max_num_children(self) -> int:
        return len(self.patterns) + 1

    def get(self, num_children: int) -> np.ndarray:
        assert num_children > 1
        if num_children - 2 >= len(self.patterns):
            raise KeyError(f"no split pattern for a 1-to-{num_children} split")
        return self.patterns[num_children - 2]


def radius_to_sphere_volume(r):
    return PI * r * r          # DimensionUtils2d (sph_kernels.rs:208-211)


def target_mass(level: np.ndarray, P: SimulationParams) -> np.ndarray:
    """LevelEstimationState::target_mass (simulation.rs:213-237), vectorised in float32.  NaN (FluidInterior) stays NaN."""
    msd, rho0 = f32(P.maximum_surface_distance), f32(P.rest_density)
    fine, base = f32(P.particle_radius_fine), f32(P.particle_radius_base)
    level = np.maximum(np.asarray(level, np.float32), -msd)
    interp = level / -msd
    one = f32(1.0)
    if P.sizing_function == "Mass":
        return (radius_to_sphere_volume(fine) * rho0) * (one - interp) + (radius_to_sphere_volume(base) * rho0) * interp
    if P.sizing_function == "Radius":
        r = fine * (one - interp) + base * interp
        return radius_to_sphere_volume(r) * rho0
    e = f32(0.5)
    r = fine * (one - np.power(interp, e, dtype=np.float32)) + base * np.power(interp, e, dtype=np.float32)
    return radius_to_sphere_volume(r) * rho0


def mass_base(P: SimulationParams) -> np.float32:
    return radius_to_sphere_volume(f32(P.particle_radius_base)) * f32(P.rest_density)     # simulation_parameters.rs:129-131


def _row_runner(kind: str, size_class, mass, level, position, h2, offsets, indices, P: SimulationParams, dt: float):
    """The body of find_share_partner_sequential (particle_sharing.rs:14-117) / find_merge_partner_sequential (particle_merging.rs:16-125)
    for ONE donor: -> (donors, run) with `donors` the particles of the donor class in ascending index and run(i, merge_partner,
    merge_counter) the walk over i's list in list order, which writes the two arrays and returns the j it claimed."""
    mass = np.asarray(mass, np.float32)
    target = target_mass(level, P)
    mbase = mass_base(P)
    share = kind == "share"
    donors = np.nonzero(np.asarray(size_class) == (LARGE if share else TOO_SMALL))[0]
    max_dist_factor = f32(P.max_share_distance if share else P.max_merge_distance)
    dtf = f32(dt)

    def run(i: int, merge_partner, merge_counter):
        claimed = []
        if share:
            dropped_i = min(mass[i] - target[i], target[i] * f32(P.max_mass_transfer_sharing) * dtf)   # dropped_mass_sharing
        else:
            dropped_i = mass[i]                                                                         # dropped_mass_merging
        for j in indices[offsets[i]:offsets[i + 1]]:
            j = int(j)
            if i == j:
                continue
            cj = size_class[j]
            if share:
                can = (cj == SMALL) or (cj == TOO_SMALL and P.allow_share_with_too_small_particle) or \
                      (cj == OPTIMAL and P.allow_share_with_optimal_particle)
            else:
                can = (cj in (SMALL, TOO_SMALL)) or (cj == OPTIMAL and P.allow_merge_with_optimal_particle)
                if P.allow_merge_on_size_difference and mass[j] > f32(5.0) * mass[i]:
                    can = True
            if not can:
                continue
            # the partner must lie within max_{share,merge}_distance mean smoothing lengths (particle_sharing.rs:60-67, particle_merging.rs:71-78)
            dx, dy = position[i, 0] - position[j, 0], position[i, 1] - position[j, 1]
            max_dist = ((h2[i] + h2[j]) * f32(0.5)) * max_dist_factor
            if dx * dx + dy * dy > max_dist * max_dist:
                continue
            new_mass_j = mass[j] + dropped_i / f32(int(merge_counter[i]) + 1)
            if new_mass_j >= target[j] * PARTICLE_SIZE_FACTOR_LARGE:
                continue
            if new_mass_j > mbase:
                continue
            if merge_partner[j] != MERGE_PARTNER_AVAILABLE:
                continue        # the neighbouring particle is being used as a partner already
            if merge_counter[i] == 0:
                if merge_partner[i] != MERGE_PARTNER_AVAILABLE:
                    continue    # this particle is itself somebody's partner
                merge_partner[i] = MERGE_PARTNER_DELETE
            merge_partner[j] = i
            merge_counter[i] += 1
            claimed.append(j)
            assert merge_counter[i] < 1000
        return claimed

    return donors, run


def _find_partners(kind: str, size_class, mass, level, position, h2, offsets, indices, P: SimulationParams, dt: float) -> Tuple[np.ndarray, np.ndarray]:
    """find_share_partner_sequential (particle_sharing.rs:14-117) / find_merge_partner_sequential (particle_merging.rs:16-125):
    the same greedy loop, in particle order, over each particle's neighbour list in list order."""
    n = len(mass)
    merge_partner = np.full(n, MERGE_PARTNER_AVAILABLE, np.uint32)
    merge_counter = np.zeros(n, np.uint16)
    donors, run = _row_runner(kind, size_class, mass, level, position, h2, offsets, indices, P, dt)
    for i in donors:
        run(int(i), merge_partner, merge_counter)
    return merge_partner, merge_counter


def find_partners_frontier(kind: str, size_class, mass, level, position, h2, offsets, indices, P: SimulationParams, dt: float):
    """The sequential loop of `_find_partners` in its exact PARALLEL schedule (the numpy twin of
    csrc/sph_partner_search.hip) -> (merge_partner, merge_counter, info), the two arrays equal to `_find_partners`'s.

    touch(i) = row(i) + {i} for a donor i with a non-empty row: everything the loop reads or writes of merge_partner while it visits i.
    writers(x): the donors whose touch set holds x, ascending.  A donor is FINISHED once it ran its row and RETIRED once it was claimed
    before it ran (the loop lets such a donor accept nobody).  head(x): the first writer of x that is neither.  Donor i is READY iff every
    x of touch(i) is claimed already (final: i skips it) or has head(x) == i.  A round runs the rows of all ready donors: no two of them
    share an unclaimed x, so the order among them does not matter, and by induction over the donor index every row sees what it sees in
    the sequential loop.  After a round, the writers of every particle claimed in it are checked again, the donors claimed in it retire,
    and head(x) moves past finished and retired writers for every x such a donor touched; the new heads are checked again.  The donors
    that are ready among those checked are the next frontier -- nothing ever sweeps over all undecided donors.

    Asserted in every round: the frontier's touch sets are disjoint on unclaimed particles, and the smallest undecided donor is in it.
    info: participants (n), candidates (the entries), donors (merge_counter > 0), transfers (the counters' sum), rounds, max_frontier,
    row_walks (rows walked by a decision or a readiness check)."""
    n = len(mass)
    AV = MERGE_PARTNER_AVAILABLE
    merge_partner = np.full(n, AV, np.uint32)
    merge_counter = np.zeros(n, np.uint16)
    donors, run = _row_runner(kind, size_class, mass, level, position, h2, offsets, indices, P, dt)
    off = np.asarray(offsets, np.int64)
    idx = np.asarray(indices, np.int64)
    donors = [int(d) for d in donors if off[d + 1] > off[d]]
    touch = {d: sorted(set(idx[off[d]:off[d + 1]].tolist()) | {d}) for d in donors}
    writers = [[] for _ in range(n)]
    for d in donors:                      # ascending, so every writers list is
        for x in touch[d]:
            writers[x].append(d)
    UNDECIDED, FINISHED, RETIRED = 0, 1, 2
    state = {d: UNDECIDED for d in donors}
    hp = [0] * n                          # head(x) = writers[x][hp[x]]
    walks = 0

    def head(x):
        return writers[x][hp[x]] if hp[x] < len(writers[x]) else -1

    def ready(i):
        nonlocal walks
        walks += 1
        return all(merge_partner[x] != AV or head(x) == i for x in touch[i])

    frontier = [d for d in donors if ready(d)]
    remaining, lo, rounds, max_frontier = len(donors), 0, 0, 0
    while frontier:
        rounds += 1
        max_frontier = max(max_frontier, len(frontier))
        while lo < len(donors) and state[donors[lo]] != UNDECIDED:
            lo += 1
        assert donors[lo] in frontier, "the smallest undecided donor is ready in every round"
        seen = set()
        for i in frontier:
            for x in touch[i]:
                if merge_partner[x] == AV:
                    assert x not in seen, "two ready donors share an unclaimed particle"
                    seen.add(x)
        claimed = []
        for i in frontier:
            claimed += run(i, merge_partner, merge_counter)
            state[i] = FINISHED
        walks += len(frontier)
        remaining -= len(frontier)
        recheck, dirty = set(), set()
        for j in claimed:
            recheck.update(writers[j])                    # (1) a claimed particle blocks none of its writers any more
            if state.get(j) == UNDECIDED:                 # (2) a claimed donor never runs
                state[j] = RETIRED
                remaining -= 1
                dirty.update(touch[j])
        for i in frontier:                                # (3) what a finished donor leaves unclaimed gets a new head
            dirty.update(x for x in touch[i] if merge_partner[x] == AV)
        for x in dirty:
            if merge_partner[x] != AV:
                continue
            while hp[x] < len(writers[x]) and state[writers[x][hp[x]]] != UNDECIDED:
                hp[x] += 1
            if head(x) >= 0:
                recheck.add(head(x))
        frontier = sorted(d for d in recheck if state[d] == UNDECIDED and ready(d))
    assert remaining == 0, f"{remaining} donors undecided and nobody ready"
    info = {"participants": n, "candidates": int(len(idx)), "donors": int(np.count_nonzero(merge_counter)), "transfers": int(merge_counter.sum()),
            "rounds": rounds, "max_frontier": max_frontier, "row_walks": walks}
    return merge_partner, merge_counter, info


def find_share_partner_sequential(size_class, mass, level, position, h2, offsets, indices, P: SimulationParams, dt: float):
    return _find_partners("share", size_class, mass, level, position, h2, offsets, indices, P, dt)


def find_merge_partner_sequential(size_class, mass, level, position, h2, offsets, indices, P: SimulationParams, dt: float):
    return _find_partners("merge", size_class, mass, level, position, h2, offsets, indices, P, dt)


def partner_candidates_reference(kind: str, size_class, mass, position, h2, offsets, indices, P: SimulationParams) -> Tuple[np.ndarray, np.ndarray]:
    """The contract of sph_download_partner_candidates (include/sph_candidates.h) in numpy float32 on a full CSR: row i is empty
    unless i is a donor of `kind` (share: Large, merge: TooSmall); a donor row keeps, in list order, every j != i that passes the two
    tests of `_find_partners` that read nothing the loop writes -- the class test (particle_sharing.rs:50-58, particle_merging.rs:57-69)
    and the distance test (particle_sharing.rs:61-65, particle_merging.rs:72-76), each f32 operation in the reference's order.
    `_find_partners` on the result takes the decisions it takes on the full lists: both tests are idempotent, the rows keep their order."""
    share = kind == "share"
    size_class = np.asarray(size_class)
    mass = np.asarray(mass, np.float32)
    position = np.asarray(position, np.float32).reshape(-1, 2)
    h2 = np.asarray(h2, np.float32)
    offsets = np.asarray(offsets, np.int64)
    indices = np.asarray(indices, np.uint32)
    n = len(mass)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    sel = np.nonzero(size_class[rows] == (LARGE if share else TOO_SMALL))[0]   # entries of donor rows
    i, j = rows[sel], indices[sel].astype(np.int64)
    keep = i != j
    cj = size_class[j]
    if share:
        can = (cj == SMALL) | ((cj == TOO_SMALL) & bool(P.allow_share_with_too_small_particle)) | \
              ((cj == OPTIMAL) & bool(P.allow_share_with_optimal_particle))
    else:
        can = (cj == SMALL) | (cj == TOO_SMALL) | ((cj == OPTIMAL) & bool(P.allow_merge_with_optimal_particle))
        if P.allow_merge_on_size_difference:
            can = can | (mass[j] > f32(5.0) * mass[i])
    keep &= can
    dx, dy = position[i, 0] - position[j, 0], position[i, 1] - position[j, 1]
    max_dist = ((h2[i] + h2[j]) * f32(0.5)) * f32(P.max_share_distance if share else P.max_merge_distance)
    keep &= ~(dx * dx + dy * dy > max_dist * max_dist)
    out_off = np.zeros(n + 1, np.uint32)
    out_off[1:] = np.cumsum(np.bincount(i[keep], minlength=n))
    return out_off, np.ascontiguousarray(indices[sel][keep])


def partner_problem_reference(kind: str, size_class, mass, level, position, h2, offsets, indices, P: SimulationParams):
    """The contract of sph_download_partner_problem (include/sph_partner_problem.h) in numpy on a full CSR and the full fields: the
    candidate rows of `partner_candidates_reference`, restricted to their PARTICIPANTS -- every donor whose row is not empty and every
    j that occurs in a row -- and renumbered by rank in ascending host index.  Returns (ids, size_class, mass, level, position, h2,
    offsets, indices): ids[K] the host indices, the five fields at ids, offsets[K + 1] / indices the participants' rows in compact
    ids (rows and entries in their order; a participant that is no donor has an empty row).  `_find_partners` with n = K on it takes
    the decisions it takes on the full lists: the renumbering is monotone, and everything the loop reads or writes belongs to a
    participant (`expand_partner_decisions` maps them back)."""
    coff, cidx = partner_candidates_reference(kind, size_class, mass, position, h2, offsets, indices, P)
    n = len(coff) - 1
    flag = np.zeros(n, bool)
    flag[np.diff(coff.astype(np.int64)) > 0] = True
    flag[cidx] = True
    ids = np.nonzero(flag)[0].astype(np.uint32)
    rank = np.cumsum(flag, dtype=np.int64) - flag          # exclusive scan of the flags
    off_c = np.append(coff[ids], np.uint32(len(cidx))).astype(np.uint32)   # every row between two participants is empty
    idx_c = rank[cidx].astype(np.uint32)
    position = np.asarray(position, np.float32).reshape(-1, 2)
    return (ids, np.asarray(size_class)[ids], np.asarray(mass, np.float32)[ids], np.asarray(level, np.float32)[ids], position[ids],
            np.asarray(h2, np.float32)[ids], off_c, idx_c)


def expand_partner_decisions(n: int, ids, mp_c, mc_c) -> Tuple[np.ndarray, np.ndarray]:
    """The numpy twin of the expand kernel (sph_share_particles_compact / sph_merge_particles_compact): merge_partner / merge_counter of
    the whole vector from the decisions on a compact problem -- AVAILABLE / 0 for everything that is no participant, a compact partner
    id mapped through `ids`, the two sentinels left alone."""
    ids = np.asarray(ids, np.int64)
    mp_c = np.asarray(mp_c, np.uint32)
    merge_partner = np.full(n, MERGE_PARTNER_AVAILABLE, np.uint32)
    merge_counter = np.zeros(n, np.uint16)
    sentinel = (mp_c == MERGE_PARTNER_AVAILABLE) | (mp_c == MERGE_PARTNER_DELETE)
    mapped = mp_c.copy()
    mapped[~sentinel] = ids[mp_c[~sentinel].astype(np.int64)]
    merge_partner[ids] = mapped
    merge_counter[ids] = np.asarray(mc_c, np.uint16)
    return merge_partner, merge_counter


def slab_partner_problem_reference(owned_ids, cand_offsets, cand_indices, size_class, mass, level, position, h2) -> dict:
    """The contract of ONE RANK's local problem (include/sph_slab_partner_problem.h) in numpy: `owned_ids` the rank's particles in the
    order of download("particle_id"), `cand_offsets` / `cand_indices` its candidate rows (one per owned particle, entries in global ids:
    sph_slab_candidates_download, or `partner_candidates_reference` on the whole vector restricted to the rank's rows), the five fields
    of the WHOLE vector by global id (what every particle's owner holds).  Participants: the owned particles with a non-empty row or
    named by an entry, in the order of `owned_ids`; behind them the entries' particles of other ranks -- here in ascending id, the
    library's order among them is its own.  -> the dict Context.slab_partner_problem_download returns."""
    owned_ids = np.asarray(owned_ids, np.int64)
    off = np.asarray(cand_offsets, np.int64)
    idx = np.asarray(cand_indices, np.uint32)
    n = len(np.asarray(mass))
    named = np.zeros(n, bool)
    named[idx] = True
    is_owned = np.zeros(n, bool)
    is_owned[owned_ids] = True
    part = (np.diff(off) > 0) | named[owned_ids]                      # by row
    foreign = np.nonzero(named & ~is_owned)[0]
    ids = np.concatenate([owned_ids[part], foreign]).astype(np.uint32)
    position = np.asarray(position, np.float32).reshape(-1, 2)
    return {"ids": ids, "n_owned": int(part.sum()), "particle_size_class": np.asarray(size_class)[ids], "mass": np.asarray(mass, np.float32)[ids],
            "level_estimation": np.asarray(level, np.float32)[ids], "position": position[ids], "h2": np.asarray(h2, np.float32)[ids],
            "offsets": np.append(off[:-1][part], off[-1]).astype(np.uint32),   # every row between two owned participants is empty
            "indices": idx.copy()}


def validate_partners(kind: str, size_class, merge_partner, merge_counter, offsets, indices) -> int:
    """validate_share_partners (particle_sharing.rs:119-150) / validate_merge_partners (particle_merging.rs:226-268)."""
    n = len(merge_counter)
    donors = 0
    want = LARGE if kind == "share" else TOO_SMALL
    for i in np.nonzero(merge_counter > 0)[0]:
        i = int(i)
        assert size_class[i] == want
        donors += 1
        assert merge_partner[i] == MERGE_PARTNER_DELETE
        nb = indices[offsets[i]:offsets[i + 1]]
        assert int((merge_partner[nb] == i).sum()) == int(merge_counter[i])
    rest = np.nonzero(merge_counter == 0)[0]
    assert not (merge_partner[rest] == MERGE_PARTNER_DELETE).any()
    recv = rest[(merge_partner[rest] != MERGE_PARTNER_AVAILABLE)]
    assert (merge_partner[merge_partner[recv]] == MERGE_PARTNER_DELETE).all()
    assert n == len(merge_partner)
    return donors


def adapt_params(P: SimulationParams, dt: float) -> ffi.SphAdaptParams:
    ap = ffi.SphAdaptParams()
    ap.dt = dt
    ap.max_mass_transfer_sharing = P.max_mass_transfer_sharing
    ap.minimum_share_partners = P.minimum_share_partners
    ap.minimum_merge_partners = P.minimum_merge_partners
    ap.fail_on_missing_split_pattern = int(P.fail_on_missing_split_pattern)
    ap.max_share_distance, ap.max_merge_distance = P.max_share_distance, P.max_merge_distance
    ap.allow_share_with_optimal_particle = int(P.allow_share_with_optimal_particle)
    ap.allow_share_with_too_small_particle = int(P.allow_share_with_too_small_particle)
    ap.allow_merge_with_optimal_particle = int(P.allow_merge_with_optimal_particle)
    ap.allow_merge_on_size_difference = int(P.allow_merge_on_size_difference)
    return ap


def find_partners_native(lib: ffi.SphLibrary, kind: str, size_class, mass, level, position, h2, offsets, indices, P: SimulationParams, dt: float, host=None):
    """The same sequential loops as `_find_partners`, compiled (sph_host_find_partners): for million-particle scenes.  `host`
    (ffi.HostBuffers): merge_partner / merge_counter land in persistent memory (views, overwritten by the next search)."""
    import ctypes as C
    n = len(mass)
    arrs = [np.ascontiguousarray(size_class, np.uint8), np.ascontiguousarray(mass, np.float32), np.ascontiguousarray(level, np.float32),
            np.ascontiguousarray(position, np.float32), np.ascontiguousarray(h2, np.float32), np.ascontiguousarray(offsets, np.uint32),
            np.ascontiguousarray(indices, np.uint32)]
    mp, mc = (np.empty(n, np.uint32), np.empty(n, np.uint16)) if host is None else (host.view("merge_partner", np.uint32, n), host.view("merge_counter", np.uint16, n))
    p, ap, tot = P.to_ffi(), adapt_params(P, dt), C.c_uint64(0)
    rc = lib.host_find_partners(0 if kind == "share" else 1, n, *[a.ctypes.data for a in arrs], C.byref(p), C.byref(ap), mp.ctypes.data, mc.ctypes.data,
                                C.byref(tot))
    if rc != 0:
        raise ffi.SphError(rc, "the partner search's validation failed (validate_share_partners / validate_merge_partners)")
    return mp, mc


class AdaptivityDriver:
    """single_step_adaptivity (simulation.rs:2732-2796) on a context that has just run single_step_without_adaptivity: sharing
    every step, merging on even step numbers, splitting on odd ones (`step_number` is FluidSimulation.step_number AFTER the step,
    :2725); mass is conserved to 0.005 (asserted like the reference).  The step's neighbour lists are read once and kept on the
    host across the passes, as the reference's NeighborhoodCache is: share_particles does not touch it, and the merge decision
    that follows still iterates the lists of the step.

    `export`: what the host reads of the lists.  "lists" (default): every neighbour list, once per step (download_neighbors).
    "candidates": per partner search, only the donors' neighbours that pass the search's class and distance tests, filtered on the
    device (download_partner_candidates, include/sph_candidates.h); the same search then takes the same decisions on those rows, and
    the two mass sums of the conservation check are reduced on the device (sum_mass).
    "compact": per partner search, the problem of its K participants only -- the donors that have a candidate and the candidates,
    renumbered 0..K-1 on the device with their five fields and their rows (download_partner_problem, include/sph_partner_problem.h);
    the same search runs with n = K and its K decisions go back through share_particles_compact / merge_particles_compact.  No full
    field and no list crosses the bus in this mode.
    "device": the same compact problem is built AND solved on the device (find_partners_device, include/sph_partner_search.h: the loop's
    exact parallel schedule, `find_partners_frontier` is its numpy twin) and share_particles_device / merge_particles_device apply the
    decisions where they are.  Per pass only the 48-byte info struct comes down and nothing goes up; the info gains "rounds" and
    "max_frontier" (the largest of the step's passes).  `DEVICE_EXPORTS` names it: `EXPORTS` stays the modes whose decisions the host takes.

    The returned info counts what crossed it: "exported_indices" (list or candidate entries), "participants" (the sum of K over the
    passes; compact mode only, else 0), "bytes_down" / "bytes_up" (the payload arrays of the step's exports and applies, computed
    from the counts: 4 B per index and offset, 21 B per particle or participant for the five fields, 6 B for the two partner
    arrays, 8 B per device mass sum)."""

    EXPORTS = ("lists", "candidates", "compact")
    DEVICE_EXPORTS = ("device",)
    INFO_BYTES = 48   # sizeof(sph_partner_search_info)

    def __init__(self, ctx: ffi.Context, split_patterns: SplitPatterns = None, log=None, export: str = "lists"):
        if export not in self.EXPORTS + self.DEVICE_EXPORTS:
            raise ValueError(f"export must be one of {self.EXPORTS + self.DEVICE_EXPORTS}, not {export!r}")
        self.ctx = ctx
        self.log = log
        self.export = export
        self.host = ffi.HostBuffers()   # the exports land in the same host memory every step (round 6: the 26 ms "download" of configs[4]'s adaptive step were mostly page faults of fresh arrays)
        if ctx.n:
            if export in ("candidates", "compact", "device"):
                self.host.reserve(ctx.n, export=export)
            else:
                self.host.reserve(ctx.n)
        if split_patterns is not None:
            ctx.set_split_patterns(split_patterns.patterns)

    def single_step_adaptivity(self, P: SimulationParams, dt: float, step_number: int, lists=None) -> dict:
        """`lists` = (offsets, indices): the step's neighbour lists when they do not live in `ctx` (slab decomposition: the ranks'
        exports assembled in global index order, distributed.group_single_step_adaptivity)."""
        import time as _t
        ctx, log = self.ctx, self.log
        candidates = self.export == "candidates"
        compact = self.export == "compact"
        device = self.export == "device"
        if (candidates or compact or device) and lists is not None:
            raise ValueError(f"export=\"{self.export}\" filters the lists that live in the context: it cannot be combined with lists= (slab assembly)")
        p, ap = P.to_ffi(), adapt_params(P, dt)
        info = {"n_before": ctx.n, "shares": 0, "merges": 0, "splits": 0, "export": self.export, "exported_indices": 0, "participants": 0,
                "bytes_down": 0, "bytes_up": 0}
        if device:
            info["rounds"] = info["max_frontier"] = 0
        # what the adaptive half of a step costs, by phase (bench.py reports it): device -> host of the lists and the five fields a
        # decision reads, the sequential partner searches on the host, the apply calls on the device
        tm = info["seconds"] = {"download": 0.0, "host_decide": 0.0, "apply": 0.0, "mass_check": 0.0}
        # particles.mass.iter().cloned().sum() (:2745, 2791) is a SEQUENTIAL f32 sum.  At the reference's own scene sizes (1e3..1e5
        # particles) that is accurate to ~1e-5 and the 0.005 bar means "mass is conserved".  At millions of particles it is not a
        # measurement any more: adding 1.8e-7 to a running total of 1.4 rounds to 1 or 2 ulp of the total every time (4M particles of
        # configs[4]: the sequential sums before and after a merge pass differ by > 0.005 although the mass is conserved to 1e-7, and
        # the reference would panic there).  The mirror keeps the assertion's MEANING: the sums are taken in f64.
        seq_sum = lambda a: float(np.sum(a, dtype=np.float64))   # noqa: E731
        t0 = _t.perf_counter()
        host = self.host
        off = idx = None
        if candidates or compact or device:
            total_mass1 = ctx.sum_mass()
            info["bytes_down"] += 8
            tm["mass_check"] += _t.perf_counter() - t0
        else:
            m1 = ctx.download("mass", host)
            off, idx = lists if lists is not None else ctx.download_neighbors(host)   # the lists single_step_without_adaptivity left behind (self.neighs)
            info["exported_indices"] += len(idx)
            info["bytes_down"] += 4 * len(m1) + (0 if lists is not None else 4 * (len(off) + len(idx)))
            t1 = _t.perf_counter()
            tm["download"] += t1 - t0
            total_mass1 = seq_sum(m1)   # (before the next download of the masses overwrites the persistent buffer)
            tm["mass_check"] += _t.perf_counter() - t1

        def decide(kind):
            nonlocal off, idx
            ta = _t.perf_counter()
            ctx.classify(p)
            t0 = _t.perf_counter()
            tm["apply"] += t0 - ta   # (classify_particles on the device: the apply side's device work)
            if compact:   # this search's participants only: their fields as they are now, their rows of the step's lists in compact ids
                _, *fields, off, idx = ctx.download_partner_problem(kind, p, ap, host)
                cls = fields[0]
                info["participants"] += len(cls)
                info["exported_indices"] += len(idx)
                info["bytes_down"] += 21 * len(cls) + 4 * (len(off) + len(idx))
                info["bytes_up"] += 6 * len(cls)
            else:
                cls = ctx.download("particle_size_class", host)
                fields = (cls, ctx.download("mass", host), ctx.download("level_estimation", host), ctx.download("position", host), ctx.download("h2", host))
                info["bytes_down"] += 21 * len(cls)
                info["bytes_up"] += 6 * len(cls)
            if candidates:   # this search's rows: the step's lists (kept on the device across share_particles), the fields as they are now
                off, idx = ctx.download_partner_candidates(kind, p, ap, host)
                info["exported_indices"] += len(idx)
                info["bytes_down"] += 4 * (len(off) + len(idx))
            t1 = _t.perf_counter()
            tm["download"] += t1 - t0
            try:
                if getattr(ctx.lib, "host_find_partners", None) is not None:
                    return find_partners_native(ctx.lib, kind, *fields, off, idx, P, dt, host)     # (validates like the reference does)
                mp, mc = _find_partners(kind, *fields, off, idx, P, dt)
                validate_partners(kind, cls, mp, mc, off, idx)
                return mp, mc
            finally:
                tm["host_decide"] += _t.perf_counter() - t1

        def apply(f, *a):
            t0 = _t.perf_counter()
            f(*a)
            tm["apply"] += _t.perf_counter() - t0

        info["passes"] = []   # per partner search: its kind, n, what it moved and its share of the `seconds` buckets

        def run_pass(kind, apply_f):
            keys = ("participants", "exported_indices", "bytes_down", "bytes_up")
            c0, t0, n0 = {k: info[k] for k in keys}, dict(tm), ctx.n
            extra = {}
            if device:   # classify, search and apply on the device: the host sees the info struct ("apply" holds all three)
                ta = _t.perf_counter()
                ctx.classify(p)
                found = ctx.find_partners_device(kind, p, ap)
                events = found["transfers"]
                info["participants"] += found["participants"]
                info["bytes_down"] += self.INFO_BYTES
                for k in ("rounds", "max_frontier"):
                    info[k] = max(info[k], found[k])
                extra = {"search": found}
                tm["apply"] += _t.perf_counter() - ta
            else:
                mp, mc = decide(kind)
                events = int(mc.sum())
            if log:
                log(f"SEQUENTIAL {kind.upper()} {events} {kind}s")
            if device:
                apply(apply_f, p, ap)
            else:
                apply(apply_f, p, ap, mp, mc)
            info["passes"].append({"kind": kind, "n": n0, "events": events, **{k: info[k] - c0[k] for k in keys}, **extra,
                                   "seconds": {k: tm[k] - t0[k] for k in ("download", "host_decide", "apply")}})
            return events

        if P.sharing:
            info["shares"] = run_pass("share", ctx.share_particles_device if device else ctx.share_particles_compact if compact else ctx.share_particles)
        if step_number % 2 == 0:
            if P.merging:
                info["merges"] = run_pass("merge", ctx.merge_particles_device if device else ctx.merge_particles_compact if compact else ctx.merge_particles)
        elif P.splitting:
            n0 = ctx.n
            apply(lambda: (ctx.classify(p), ctx.split_particles(p, ap)))
            info["splits"] = ctx.n - n0
        t0 = _t.perf_counter()
        if candidates or compact or device:
            total_mass2 = ctx.sum_mass()
            info["bytes_down"] += 8
            tm["mass_check"] += _t.perf_counter() - t0
        else:
            m2 = ctx.download("mass", host)
            info["bytes_down"] += 4 * len(m2)
            t1 = _t.perf_counter()
            tm["download"] += t1 - t0
            total_mass2 = seq_sum(m2)
            tm["mass_check"] += _t.perf_counter() - t1
        if not abs(total_mass1 - total_mass2) <= 0.005:             # assert_ft_approx_eq(total_mass1, total_mass2, 0.005, "mass sum")
            raise AssertionError(f"mass sum: {total_mass1} vs {total_mass2}")
        info["n_after"] = ctx.n
        return info
