"""The compact partner problem of a slab decomposition on the host (no GPU, no library): adaptivity.slab_partner_problem_reference -- the
contract of ONE rank's local problem (include/sph_slab_partner_problem.h) -- per rank, then distributed.merge_slab_partner_problems,
against adaptivity.partner_problem_reference on the whole vector, array for array; and `_find_partners` on the merged problem, expanded
by adaptivity.expand_partner_decisions, against `_find_partners` on the full lists, for every parameter case of
tests/test_partner_problem_host.py.

The vector is synthetic: a jittered 20 x 15 grid, random classes, masses around the target mass of random levels, and as lists random
subsets of the particles within three spacings, ascending.  The "ranks" are slabs in x with their owned particles in a shuffled order
(a rank's rows are not sorted by id); rows near a cut name the other rank's particles.  The strip x > 0.9 holds TooLarge particles only
-- nobody's donor -- so the rank that owns exactly that strip has an empty local problem."""
import numpy as np
import pytest

from adaptive_sph_amd import adaptivity as A, distributed as D
from adaptive_sph_amd.workloads import default_params

RADII = dict(particle_radius_fine=0.012, particle_radius_base=0.05, maximum_surface_distance=0.3)
ALLOW = ["allow_share_with_optimal_particle", "allow_share_with_too_small_particle", "allow_merge_with_optimal_particle",
         "allow_merge_on_size_difference"]
CASES = [{}] + [{a: True} for a in ALLOW] + [{"max_share_distance": d, "max_merge_distance": d} for d in (0.5, 2.0)]   # tests/test_partner_problem_host.py
FIELDS = ("particle_size_class", "mass", "level_estimation", "position", "h2")
KINDS = ("share", "merge")
PARTITIONS = {"two": [0.5], "three": [0.33, 0.66], "three_one_idle": [0.45, 0.9], "two_one_idle": [0.9]}
DT = 1e-3


@pytest.fixture(scope="module")
def vector():
    rng = np.random.default_rng(20261019)
    nx, ny = 20, 15
    n = nx * ny
    d = 1.0 / nx
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    pos = (np.stack([gx.ravel(), gy.ravel()], 1) + 0.5 + rng.uniform(-0.3, 0.3, (n, 2))) * d
    perm = rng.permutation(n)                         # ids do not follow x
    pos = pos[perm].astype(np.float32)
    P = default_params(**RADII)
    level = rng.uniform(-0.3, 0.0, n).astype(np.float32)
    mass = (A.target_mass(level, P) * rng.uniform(0.3, 2.5, n)).astype(np.float32)
    cls = rng.integers(0, 5, n).astype(np.uint8)
    cls[pos[:, 0] > 0.9] = A.TOO_LARGE
    h2 = (2.0 * d * rng.uniform(0.8, 1.2, n)).astype(np.float32)
    rows = []
    for i in range(n):
        near = np.nonzero(np.hypot(*(pos - pos[i]).T) < 3 * d)[0]
        rows.append(np.sort(rng.choice(near, size=max(1, int(len(near) * 0.7)), replace=False)))
    off = np.zeros(n + 1, np.uint32)
    off[1:] = np.cumsum([len(r) for r in rows])
    idx = np.concatenate(rows).astype(np.uint32)
    f = {"particle_size_class": cls, "mass": mass, "level_estimation": level, "position": pos, "h2": h2}
    return P, f, off, idx, rng


def owned_of(f, cuts, rng):
    """the ranks' owned ids, each in an order of its own"""
    edges = [-np.inf] + list(cuts) + [np.inf]
    x = f["position"][:, 0]
    return [rng.permutation(np.nonzero((x >= lo) & (x < hi))[0]).astype(np.uint32) for lo, hi in zip(edges[:-1], edges[1:])]


def local_problems(kind, P, f, off, idx, owned):
    coff, cidx = A.partner_candidates_reference(kind, f["particle_size_class"], f["mass"], f["position"], f["h2"], off, idx, P)
    parts = []
    for ids in owned:
        rows = [cidx[coff[i]:coff[i + 1]] for i in ids]
        roff = np.zeros(len(ids) + 1, np.uint32)
        roff[1:] = np.cumsum([len(r) for r in rows])
        ridx = np.concatenate(rows + [np.empty(0, np.uint32)]).astype(np.uint32)
        parts.append(A.slab_partner_problem_reference(ids, roff, ridx, *[f[k] for k in FIELDS]))
    return parts, (coff, cidx)


def assert_same_problem(got, want):
    assert len(got) == len(want) == 8
    for name, a, b in zip(("ids",) + FIELDS + ("offsets", "indices"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), name


@pytest.mark.parametrize("partition", sorted(PARTITIONS))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("over", CASES, ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()) or "default")
def test_merged_local_problems_are_the_problem_of_the_whole_vector(vector, partition, kind, over):
    P, f, off, idx, _ = vector
    P = P.replace(**over)
    n = len(f["mass"])
    owned = owned_of(f, PARTITIONS[partition], np.random.default_rng(7))
    assert sum(len(o) for o in owned) == n and all(len(o) for o in owned)
    parts, _ = local_problems(kind, P, f, off, idx, owned)
    want = A.partner_problem_reference(kind, *[f[k] for k in FIELDS], off, idx, P)
    got = D.merge_slab_partner_problems(parts)
    assert_same_problem(got, want)
    for dense in (True, False):                                      # both ways from an id to its compact id
        assert_same_problem(D.merge_slab_partner_problems(parts, dense=dense), want)
    K = len(want[0])
    assert 0 < K < n
    owner = np.empty(n, np.int64)
    for r, o in enumerate(owned):
        owner[o] = r
    for r, q in enumerate(parts):                                    # the structure the header states
        ko = q["n_owned"]
        assert np.all(owner[q["ids"][:ko]] == r) and np.all(owner[q["ids"][ko:]] != r)
        assert len(q["offsets"]) == ko + 1 and int(q["offsets"][-1]) == len(q["indices"])
        assert np.isin(q["indices"], q["ids"]).all() and len(np.unique(q["ids"])) == len(q["ids"])
        pos_in_owned = {int(i): k for k, i in enumerate(owned[r])}
        order = [pos_in_owned[int(i)] for i in q["ids"][:ko]]
        assert order == sorted(order)                                # owned participants in the rank's row order
    if "idle" in partition:
        assert len(parts[-1]["ids"]) == 0 and parts[-1]["n_owned"] == 0 and parts[-1]["offsets"].tolist() == [0]
    wide = over.get("max_share_distance", 1.0) >= 1.0                # (half the distance keeps too few pairs to demand one across every cut)
    if partition in ("two", "three") and wide:
        assert any(len(q["ids"]) > q["n_owned"] for q in parts)      # some row crosses a cut
    if partition == "three" and wide:
        mid = parts[1]["ids"][parts[1]["n_owned"]:]
        assert {int(o) for o in owner[mid]} == {0, 2}                # the middle rank has foreign participants on both sides
    # the decisions
    full = A._find_partners(kind, *[f[k] for k in FIELDS], off, idx, P, DT)
    ids, *fields_c, off_c, idx_c = got
    mp_c, mc_c = A._find_partners(kind, *fields_c, off_c, idx_c, P, DT)
    A.validate_partners(kind, fields_c[0], mp_c, mc_c, off_c, idx_c)
    mp, mc = A.expand_partner_decisions(n, ids, mp_c, mc_c)
    assert np.array_equal(full[0], mp) and np.array_equal(full[1], mc)
    if not over:
        assert int(full[1].sum()) > 0


@pytest.mark.parametrize("partition", ["two", "three"])
def test_a_kind_without_participants(vector, partition):
    """nobody is Large: the share problem is empty on every rank and as a whole"""
    P, f, off, idx, _ = vector
    f = dict(f)
    f["particle_size_class"] = np.where(f["particle_size_class"] == A.LARGE, A.OPTIMAL, f["particle_size_class"]).astype(np.uint8)
    owned = owned_of(f, PARTITIONS[partition], np.random.default_rng(7))
    parts, _ = local_problems("share", P, f, off, idx, owned)
    assert all(len(q["ids"]) == 0 for q in parts)
    got = D.merge_slab_partner_problems(parts)
    assert_same_problem(got, A.partner_problem_reference("share", *[f[k] for k in FIELDS], off, idx, P))
    assert len(got[0]) == 0 and got[6].tolist() == [0] and len(got[7]) == 0
    mp, mc = A.expand_partner_decisions(len(f["mass"]), got[0], np.zeros(0, np.uint32), np.zeros(0, np.uint16))
    assert np.all(mp == A.MERGE_PARTNER_AVAILABLE) and not mc.any()
    parts, _ = local_problems("merge", P, f, off, idx, owned)          # ... while the merge problem of the same vector is not
    assert_same_problem(D.merge_slab_partner_problems(parts), A.partner_problem_reference("merge", *[f[k] for k in FIELDS], off, idx, P))


@pytest.mark.parametrize("field", FIELDS)
def test_two_ranks_that_disagree_on_a_particle_are_refused(vector, field):
    """a stale ghost: rank 1 reports a particle of rank 0 with another value than its owner -- the merge raises, it does not pick one"""
    P, f, off, idx, _ = vector
    owned = owned_of(f, PARTITIONS["two"], np.random.default_rng(7))
    parts, _ = local_problems("merge", P, f, off, idx, owned)
    q0, q1 = parts
    shared = np.intersect1d(q0["ids"][:q0["n_owned"]], q1["ids"][q1["n_owned"]:])
    assert len(shared) > 0
    k = int(np.nonzero(q1["ids"] == shared[0])[0][0])
    bad = {key: (v.copy() if isinstance(v, np.ndarray) else v) for key, v in q1.items()}
    if field == "particle_size_class":
        bad[field][k] = (bad[field][k] + 1) % 5
    else:
        bad[field][k] = np.nextafter(bad[field][k], np.float32(np.inf))
    for dense in (None, True, False):
        with pytest.raises(ValueError, match=str(int(shared[0]))):
            D.merge_slab_partner_problems([q0, bad], dense=dense)
    D.merge_slab_partner_problems([q0, q1])


def test_malformed_parts_are_refused(vector):
    P, f, off, idx, _ = vector
    owned = owned_of(f, PARTITIONS["two"], np.random.default_rng(7))
    parts, _ = local_problems("merge", P, f, off, idx, owned)
    with pytest.raises(ValueError, match="owned by two ranks"):
        D.merge_slab_partner_problems([parts[0], parts[0]])
    q = dict(parts[1])
    union = np.union1d(parts[0]["ids"], parts[1]["ids"])
    stranger = np.setdiff1d(np.arange(len(f["mass"]), dtype=np.uint32), union)[0]
    q["indices"] = q["indices"].copy()
    q["indices"][0] = stranger                                       # an entry that names nobody's participant
    for dense in (True, False):
        with pytest.raises(ValueError, match="no participant"):
            D.merge_slab_partner_problems([parts[0], q], dense=dense)
    q["indices"][0] = 10 ** 6                                        # ... or nobody at all
    for dense in (True, False):
        with pytest.raises(ValueError, match="no participant"):
            D.merge_slab_partner_problems([parts[0], q], dense=dense)
    q = dict(parts[1])
    q["offsets"] = q["offsets"][:-1]
    with pytest.raises(ValueError, match="offsets"):
        D.merge_slab_partner_problems([parts[0], q])


def test_symbols_and_header(product_lib, oracle_lib):
    """what the header declares is what ffi.py binds; the oracle has none of it; export="compact" is a mode of both slab drivers"""
    import re
    from pathlib import Path
    from adaptive_sph_amd import ffi
    header = (Path(__file__).resolve().parent.parent / "include" / "sph_slab_partner_problem.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sph_[a-z_0-9]+)\s*\(", header)))
    assert declared == sorted("sph_" + s for s in ffi.SLAB_PROBLEM_SYMBOLS)
    for s in ffi.SLAB_PROBLEM_SYMBOLS:
        assert hasattr(product_lib.lib, "sph_" + s), s
        assert s not in ffi.ABI_SYMBOLS and s not in ffi.SLAB_CANDIDATE_SYMBOLS and s not in ffi.PROBLEM_SYMBOLS
        assert getattr(product_lib, s) is not None and getattr(oracle_lib, s) is None
    assert D.SLAB_EXPORTS == ("lists", "candidates", "compact")
    with pytest.raises(ValueError):
        D.group_single_step_adaptivity_on_slabs(product_lib, [], default_params(), 1e-3, 2, export="everything")
