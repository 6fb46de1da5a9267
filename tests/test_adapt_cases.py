"""The designed cases of tests/adapt_cases.py on the CPU: the oracle (oracle/adapt.c) against the sequential models bit for bit, and
every case against the branch it is named after -- n_del, n_new mod 256, the plateaus of the prefix sum, both arms of the min, the tie
itself.  A case that stops hitting its branch fails here, not silently on the GPU (tests/test_gpu_adapt_branch_points.py).  No GPU."""
import numpy as np
import pytest

from adaptive_sph_amd import adaptivity as A, ffi, scene as sc
from tests import adapt_cases as AC

f32 = np.float32
MERGE = AC.merge_cases()
SHARE = AC.share_cases()
SPLIT = AC.split_cases()
ids = lambda cases: [c.name for c in cases]
upload, check_slab_transfer_case, check_slab_split_case = AC.upload, AC.check_slab_transfer_case, AC.check_slab_split_case


def closed_form(n, deleted, rank_shift=0, tail_shift=0):
    """sph_adapt.hip's statement of the swap loop: the k-th hole from the front receives the k-th survivor from the back.
    rank_shift / tail_shift: the same formula off by one (a survivor's rank, the first index of the tail), for the sensitivity test"""
    d = np.zeros(n, bool)
    d[deleted] = True
    n_del = int(d.sum())
    n_new = n - n_del
    ident = np.arange(n)
    holes = np.nonzero(d[:n_new])[0]
    before = np.cumsum(d) - d                                     # exclusive prefix of the delete flags
    tail = []
    for t in range(max(n_new + tail_shift, 0), n):
        if d[t]:
            continue
        rank = (n - 1 - t) - (n_del - before[t] - d[t]) + rank_shift
        if 0 <= rank < len(holes):
            ident[holes[rank]] = t
            tail.append(t)
    return ident[:n_new], holes, np.asarray(tail[::-1], np.int64)


def check_merge(oracle_lib, c):
    P = c.params()
    o = upload(oracle_lib, c)
    o.merge_particles(P.to_ffi(), c.adapt_params(), c.merge_partner, c.merge_counter)
    m, x, v, hn, ident = AC.merge_model(c.mass, c.position, c.velocity, c.h2_next, c.merge_partner, c.merge_counter, int(P.minimum_merge_partners), P.rest_density)
    assert o.n == len(m) == c.note["n_new"]
    got = {f: o.download(f) for f in AC.FIELDS}
    assert np.array_equal(got["level_old"], ident.astype(np.float32))                    # the slot order of the survivors
    assert np.array_equal(got["mass"], m) and np.array_equal(got["position"], x) and np.array_equal(got["velocity"], v) and np.array_equal(got["h2_next"], hn)
    for f, src in (("h2", c.h2), ("level_estimation", c.level), ("particle_size_class", c.size_class)):
        assert np.array_equal(got[f], src[ident]), f                                       # carried with their particle
    cf, holes, tail = closed_form(c.n, c.note["deleted"])
    assert np.array_equal(cf, ident)                                                       # what the device computes instead of the loop
    return ident, holes, tail


@pytest.mark.parametrize("c", MERGE, ids=ids(MERGE))
def test_merge_cases(oracle_lib, c):
    ident, holes, tail = check_merge(oracle_lib, c)
    n, n_new, n_del, deleted = c.n, c.note["n_new"], c.note["n_del"], c.note["deleted"]
    assert n_new + n_del == n
    name = c.name
    if name == "tail only":
        assert deleted.min() >= n_new and len(holes) == 0
    elif name == "head only":
        assert deleted.max() < n_new and len(holes) == n_del and np.array_equal(tail, np.arange(n - 1, n_new - 1, -1))
    elif name == "last k + scattered":
        assert all(i in deleted for i in range(n - 17, n)) and 0 < len(holes) < n_del
    elif name.startswith("all but"):
        assert n_new == 1 and n_del == n - 1
    elif name == "everything":
        assert n_new == 0 and n_del == n
    elif name == "n = 1":
        assert n == 1 and n_new == 0
    elif name == "n = 1, kept":
        assert n == 1 and n_new == 1
    elif name == "n = 2":
        assert n == 2 and n_new == 1 and ident[0] == 1
    elif name.startswith("minimum partners"):
        kept = np.nonzero((c.merge_partner == AC.DEL) & (c.merge_counter < 2))[0]
        assert len(kept) and (kept >= n_new).any() and len(holes)                           # donors that stay, inside the tail, moved into holes
    elif name.startswith("n_new = 256"):
        assert n_new == 256 and n_del == int(name.split("=")[-1])
    elif name.startswith("n = "):
        assert n == int(name.split(",")[0].split("=")[1])
        for t in range(AC.SCAN_TILE, n, AC.SCAN_TILE):
            assert t - 1 in deleted or c.merge_partner[t - 1] == AC.DEL
            assert c.merge_partner[t] == AC.DEL
        assert {int(k) for k in np.unique(c.merge_counter[c.merge_partner == AC.DEL])} >= ({1, 2, 3} if "= 0" in name.split(",")[1] else {1, 2})
        if "= 2" in name.split(",")[1]:
            stay = np.nonzero((c.merge_partner == AC.DEL) & (c.merge_counter < 2))[0]
            assert len(stay) > 3 and not np.isin(stay, deleted).any()


@pytest.mark.parametrize("mutant", [dict(rank_shift=1), dict(rank_shift=-1)], ids=str)
def test_merge_cases_tell_an_off_by_one_in_the_closed_form(mutant):
    """The index arithmetic is not mutated on the device (a wrong index reads or writes out of bounds there): the closed form with a
    survivor's rank or the tail's first index off by one differs from the right one in most cases that have a hole."""
    with_holes = [c for c in MERGE if len(closed_form(c.n, c.note["deleted"])[1])]
    caught = [c.name for c in with_holes if not np.array_equal(closed_form(c.n, c.note["deleted"], **mutant)[0], closed_form(c.n, c.note["deleted"])[0])]
    assert len(with_holes) >= 10 and len(caught) >= len(with_holes) - 3, (caught, [c.name for c in with_holes])


def test_merge_cases_cover_the_receiver_counts_and_minimum_partners():
    counts = set()
    for c in MERGE:
        counts |= {int(k) for k in np.unique(c.merge_counter[c.merge_partner == AC.DEL])}
    assert counts >= {0, 1, 2, 3}
    assert {c.params().minimum_merge_partners for c in MERGE} == {0, 2}
    assert any(c.note["n_new"] % 256 == 0 and c.note["n_new"] for c in MERGE) and any(c.note["n_del"] % 256 == 0 and c.note["n_del"] for c in MERGE)


def test_merge_receivers_of_a_donor_that_stays_are_untouched(oracle_lib):
    c = next(c for c in MERGE if c.name.startswith("minimum partners"))
    P = c.params()
    o = upload(oracle_lib, c)
    o.merge_particles(P.to_ffi(), c.adapt_params(), c.merge_partner, c.merge_counter)
    tag = o.download("level_old").astype(np.int64)
    stay = np.nonzero((c.merge_partner == AC.DEL) & (c.merge_counter < 2))[0]
    recv = np.nonzero(np.isin(c.merge_partner, stay))[0]
    assert len(stay) and len(recv)
    for i in np.concatenate([stay, recv]):
        slot = np.nonzero(tag == i)[0]
        assert len(slot) == 1
        for f, src in (("mass", c.mass), ("position", c.position), ("velocity", c.velocity), ("h2_next", c.h2_next)):
            assert np.array_equal(o.download(f)[slot[0]], src[i]), f


def test_merge_case_with_a_chunked_scan_carry(oracle_lib):
    """n = 524 289: 257 tiles, so the scan of the tile sums (k_scan_sums) carries from its first chunk of 256 into a second one"""
    c = AC.merge_case_large()
    n_tiles = -(-c.n // AC.SCAN_TILE)
    assert n_tiles == AC.SCAN_BLOCK + 1
    deleted = c.note["deleted"]
    assert deleted.min() < AC.SCAN_TILE and deleted.max() >= (n_tiles - 1) * AC.SCAN_TILE     # a donor in the first and in the last tile
    assert np.count_nonzero(deleted >= (n_tiles - 1) * AC.SCAN_TILE) == 1                     # the carry into the last tile is everything before it
    P = c.params()
    o = upload(oracle_lib, c)
    o.merge_particles(P.to_ffi(), c.adapt_params(), c.merge_partner, c.merge_counter)
    ident, holes, tail = closed_form(c.n, deleted)
    assert o.n == c.note["n_new"] and np.array_equal(o.download("level_old"), ident.astype(np.float32))
    # the receivers' values: the model's first loop, vectorised (one receiver per donor)
    r = np.nonzero(c.merge_partner < AC.DEL)[0]
    d = c.merge_partner[r].astype(np.int64)
    m = c.mass.copy()
    m[r] = c.mass[r] + c.mass[d] / f32(1)
    x = c.position.copy()
    x[r] = (c.mass[r, None] * c.position[r] + c.mass[d, None] * c.position[d]) / m[r, None]
    assert np.array_equal(o.download("mass"), m[ident]) and np.array_equal(o.download("position"), x[ident])
    # a carry that forgot the first chunk would shift the last tile's donor: its rank among the deleted is n_del - 1
    assert np.searchsorted(deleted, c.n - 1) == c.note["n_del"] - 1 > AC.SCAN_BLOCK * 3


@pytest.mark.parametrize("c", SHARE, ids=ids(SHARE))
def test_share_cases(oracle_lib, c):
    P = c.params()
    o = upload(oracle_lib, c)
    o.share_particles(P.to_ffi(), c.adapt_params(), c.merge_partner, c.merge_counter)
    mp = int(P.minimum_share_partners)
    m, x, v, hn, arms = AC.share_model(c.mass, c.position, c.velocity, c.h2_next, c.level, c.merge_partner, c.merge_counter, mp, P, c.dt)
    assert o.n == c.n
    for f, want in (("mass", m), ("position", x), ("velocity", v), ("h2_next", hn), ("h2", c.h2), ("level_old", c.level_old), ("particle_size_class", c.size_class)):
        assert np.array_equal(o.download(f), want), f
    assert np.array_equal(o.download("level_estimation"), c.level)
    # both arms of the min, at every level of the design -- above, at and below the clamp
    msd = f32(AC.MSD)
    seen = {(int(arm), int(np.digitize(-c.level[d] / msd, [0.25, 0.75, 1.5]))) for d, arm in arms.items()}
    assert seen == {(a, l) for a in (0, 1) for l in range(4)}, seen
    target = A.target_mass(c.level, P)
    below = [d for d in arms if c.level[d] < -msd]
    assert below and all(target[d] == A.target_mass(np.asarray([-msd], np.float32), P)[0] for d in below)    # the fmaxf clamp acts
    gave = np.asarray(sorted(arms))
    assert (m[gave] < c.mass[gave]).all() and (m[gave] >= target[gave]).all()
    if mp == 2:
        stay = np.nonzero((c.merge_partner == AC.DEL) & (c.merge_counter < 2))[0]
        recv = np.nonzero(np.isin(c.merge_partner, stay))[0]
        assert len(stay) and len(recv) and np.array_equal(m[stay], c.mass[stay]) and np.array_equal(x[recv], c.position[recv])
    assert {int(k) for k in np.unique(c.merge_counter[c.merge_partner == AC.DEL])} == {1, 2, 3}
    # the swapped comparison (fmaxf for fminf) gives another mass at every donor
    t2 = f32(P.max_mass_transfer_sharing) * f32(c.dt)
    other = c.mass[gave] - np.maximum(c.mass[gave] - target[gave], target[gave] * f32(P.max_mass_transfer_sharing) * f32(c.dt))
    assert t2 < 1 and (other != m[gave]).all()


@pytest.mark.parametrize("c", SPLIT, ids=ids(SPLIT))
def test_split_cases(oracle_lib, c):
    P = c.params()
    sp = A.SplitPatterns.load_from_file(AC.PATTERNS)
    assert sp.get_max_num_children() == 59
    patterns = sp.patterns if c.patterns else []
    o = upload(oracle_lib, c)
    o.set_split_patterns(patterns)
    status, want = AC.split_model(c, patterns, c.capacity)
    assert status == c.status
    if status:
        with pytest.raises(ffi.SphError) as e:
            o.split_particles(P.to_ffi(), c.adapt_params())
        assert e.value.status == status
    else:
        o.split_particles(P.to_ffi(), c.adapt_params())
        assert o.n == c.n + c.note["extra"] == len(want["mass"])
        for f in AC.FIELDS:
            assert np.array_equal(o.download(f), want[f], equal_nan=f == "level_estimation"), f
    found, parents = c.note["found"], c.note["parents"]
    target = A.target_mass(c.level, P)
    for ratio, where in found.items():
        for i in where:
            assert np.isnan(c.level[i]) or f32(c.mass[i]) / target[i] == f32(ratio)                                # the tie itself
    name = c.name
    if name.startswith("ties") or name.startswith("capacity") or name.startswith("n = 2049") or name.startswith("Radius2"):
        assert set(found) == set(AC.TIES)
        even_half = [i for r in (2.5, 58.5) for i in found[r]]                              # where roundf and rintf part
        assert even_half and all(AC.round_half_away(c.mass[i] / target[i]) != np.rint(c.mass[i] / target[i]) for i in even_half)
        kids = {r: AC.num_children(c.mass[found[r][0]], target[found[r][0]], 59, False) for r in found}
        assert kids == {1.5: 2, 2.5: 3, 3.5: 4, 58.5: 59, 59.5: 59}                          # 59.5 rounds to 60 and clamps to the table
        # plateaus of the exclusive prefix on both sides of the binary search: parents at 0 and n - 1, runs of neighbours, gaps
        assert parents[0] == 0 and (parents[-1] == c.n - 1 or name.startswith("n = 2049")) and (np.diff(parents) == 1).any() and (np.diff(parents) > 1).any()
    if name.startswith("59.5 refused"):
        assert 59.5 in found and P.fail_on_missing_split_pattern
    if name.startswith("1.4999999"):
        assert AC.JUST_BELOW in found and AC.JUST_BELOW < 1.5 and AC.num_children(c.mass[found[AC.JUST_BELOW][0]], target[found[AC.JUST_BELOW][0]], 59, False) is None
    if name == "capacity of exactly n + extra":
        assert c.capacity == c.n + c.note["extra"]
    if name == "capacity one short":
        assert c.capacity == c.n + c.note["extra"] - 1
    if name.startswith("a NaN"):
        assert np.isnan(c.level[parents]).sum() == 1
    if name.startswith("n = 2049"):
        assert {2046, 2047, 2048} <= set(parents.tolist())
    if name.startswith("Radius2"):
        interp = np.maximum(c.level[parents], -f32(AC.MSD)) / -f32(AC.MSD)
        assert set(np.unique(interp).tolist()) == {0.0, 1.0}


def parent_of_child(base, c, strict=False, lo_mid=False):
    """k_split_plan's binary search: the last index whose exclusive prefix sum is <= c.  strict / lo_mid: the same search with `<` for `<=`,
    or with the midpoint rounded down and `lo = mid + 1` (the first index instead of the last), for the sensitivity test"""
    lo, hi = 0, len(base) - 1
    while lo < hi:
        if lo_mid:
            mid = (lo + hi) >> 1
            if base[mid] < c:
                lo = mid + 1
            else:
                hi = mid
        else:
            mid = (lo + hi + 1) >> 1
            if (base[mid] < c) if strict else (base[mid] <= c):
                lo = mid
            else:
                hi = mid - 1
    return lo


def test_split_cases_tell_an_off_by_one_in_the_parent_search():
    """The binary search is not mutated on the device.  Here: the search as the kernel states it finds every child's parent in the order the
    sequential loop appends them -- across the plateaus the non-parents leave in the prefix sum -- and its off-by-one forms do not."""
    sp = A.SplitPatterns.load_from_file(AC.PATTERNS)
    checked = 0
    for c in SPLIT:
        if c.status or not c.note["extra"]:
            continue
        target = A.target_mass(c.level, c.params())
        extra = np.zeros(c.n, np.int64)
        for i in c.note["parents"]:
            extra[i] = AC.num_children(c.mass[i], target[i], sp.get_max_num_children(), False) - 1
        base = np.cumsum(extra) - extra
        want = np.repeat(np.arange(c.n), extra)                          # the parent of appended child 0, 1, ... in the loop's order
        got = [parent_of_child(base, k) for k in range(len(want))]
        assert np.array_equal(got, want)
        assert (np.diff(base) == 0).sum() > c.n // 2 and base[0] == 0 and extra[0] > 0 and (extra[-1] > 0 or c.n == 2049)   # plateaus on both sides
        for mutant in (dict(strict=True), dict(lo_mid=True)):
            assert not np.array_equal([parent_of_child(base, k, **mutant) for k in range(len(want))], want), mutant
        checked += 1
    assert checked >= 5


# ---- the slab cases, built here from the oracle's neighbour lists (on the device: from the group's own) --------------------------
def slab_world(oracle_lib, k, interleaved):
    from adaptive_sph_amd import distributed as D
    pos, mass, vel, planes = AC.slab_scene(interleaved)
    o = ffi.Context(oracle_lib, len(mass), planes)
    o.upload(mass, pos, vel)
    o.step(AC.dam_break_params(level_estimation_method="None").to_ffi())
    f = {name: o.download(name) for name in ("mass", "position", "velocity", "h2", "h2_next")}
    cuts = D.slab_cuts(pos[:, 0], k)
    rank = AC.slab_rank_of(D.partition(f["position"][:, 0], cuts), len(mass))
    off, idx = o.download_neighbors()
    return f, cuts, rank, off.astype(np.int64), idx


@pytest.mark.parametrize("k", [2, 3, 4])
def test_slab_transfer_cases(oracle_lib, k):
    f, cuts, rank, off, idx = slab_world(oracle_lib, k, False)
    assert all(np.all(np.diff(np.nonzero(rank == r)[0]) == 1) for r in range(k))           # the scene's order: contiguous ids per rank
    specs = AC.slab_transfer_cases(len(rank), rank, off, idx, f["mass"])
    assert len(specs) == 5
    for spec in specs:
        c = AC.slab_case(spec, **f)
        recv = np.nonzero(c.merge_partner < AC.DEL)[0]
        assert all(c.merge_partner[r] in idx[off[r]:off[r + 1]] for r in recv)                # every donor is a neighbour of its receivers
        check_slab_transfer_case(c, rank)
        if c.kind == "merge":
            c.note["deleted"] = np.nonzero((c.merge_partner == AC.DEL) & (c.merge_counter >= c.params().minimum_merge_partners))[0]
            c.note["n_new"] = c.n - len(c.note["deleted"])
            check_merge(oracle_lib, c)
        else:
            P = c.params()
            o = upload(oracle_lib, c)
            o.share_particles(P.to_ffi(), c.adapt_params(), c.merge_partner, c.merge_counter)
            m, x, v, hn, arms = AC.share_model(c.mass, c.position, c.velocity, c.h2_next, c.level, c.merge_partner, c.merge_counter, 0, P, c.dt)
            for name, want in (("mass", m), ("position", x), ("velocity", v), ("h2_next", hn)):
                assert np.array_equal(o.download(name), want), name
            assert set(arms.values()) == {0, 1} and (m[sorted(arms)] < c.mass[sorted(arms)]).all()


@pytest.mark.parametrize("k", [2, 3, 4])
def test_slab_split_cases(oracle_lib, k):
    f, cuts, rank, off, idx = slab_world(oracle_lib, k, True)
    assert (np.diff(rank[:200]) != 0).mean() > 0.3                                         # interleaved ids
    sp = A.SplitPatterns.load_from_file(AC.PATTERNS)
    for spec in AC.slab_split_cases(len(rank), rank, f["position"], f["mass"], cuts):
        c = AC.slab_case(spec, **f)
        check_slab_split_case(c, rank)
        target = A.target_mass(c.level, c.params())
        assert all(f32(c.mass[i]) / target[i] == f32(r) for i, r in spec["ratios"].items()) and {2.5, 59.5} <= set(spec["ratios"].values())
        o = upload(oracle_lib, c)
        o.set_split_patterns(sp.patterns)
        status, want = AC.split_model(c, sp.patterns, c.capacity)
        assert status == 0
        o.split_particles(c.params().to_ffi(), c.adapt_params())
        for name in AC.FIELDS:
            assert np.array_equal(o.download(name), want[name]), name
