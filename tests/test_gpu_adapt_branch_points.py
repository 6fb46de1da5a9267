"""The apply half of single_step_adaptivity on the device (csrc/sph_adapt.hip: sph_share_particles / sph_merge_particles / sph_split_particles
and their slab forms) at the designed cases of tests/adapt_cases.py, against the CPU oracle on IDENTICAL inputs, bit for bit: the library and
the oracle are built with -ffp-contract=off and every operation of the apply is one IEEE f32 operation in the reference's order, so nothing
here is a tolerance.  tests/test_adapt_cases.py checks on the CPU that the oracle agrees with the sequential models on these cases and that
every case hits the branch it is named after."""
import numpy as np
import pytest

from adaptive_sph_amd import adaptivity as A, distributed as D, ffi
from tests import adapt_cases as AC

pytestmark = pytest.mark.gpu
SP = A.SplitPatterns.load_from_file(AC.PATTERNS)
MERGE, SHARE, SPLIT = AC.merge_cases(), AC.share_cases(), AC.split_cases()
APPLIED = [c for c in MERGE + SHARE + SPLIT if c.status == 0]
REFUSED = [c for c in SPLIT if c.status != 0]
ids = lambda cases: [f"{c.kind}: {c.name}" for c in cases]


def _planes():
    from adaptive_sph_amd import scene as sc
    return sc.boundary_planes(sc.dam_break_small().boundary)


def apply(ctx, c):
    p, ap = c.params().to_ffi(), c.adapt_params()
    if c.kind == "split":
        ctx.split_particles(p, ap)
    else:
        (ctx.share_particles if c.kind == "share" else ctx.merge_particles)(p, ap, c.merge_partner, c.merge_counter)


def pair(product_lib, oracle_lib, c, order):
    """the case on the product and on the oracle.  cold: straight after upload + upload_field (orig is the identity).  permuted: the product
    steps first, so that orig is the cell sort's permutation and slot_of is exercised; its fields become the oracle's upload, the designed
    level and class fields are written to both sides afterwards."""
    g = AC.upload(product_lib, c)
    if order == "permuted":
        g.step(c.params().to_ffi())
        if c.n > 64:
            assert (np.diff(g.download("cell_index").astype(np.int64)) < 0).any()          # host order is not cell order
        moved = {f: g.download(f) for f in ("mass", "position", "velocity", "h2", "h2_next")}
        assert np.array_equal(moved["mass"], c.mass)
        o = ffi.Context(oracle_lib, c.capacity, _planes())
        o.upload(moved["mass"], moved["position"], moved["velocity"])
        for f in ("h2", "h2_next"):
            o.upload_field(f, moved[f])
        for f, v in (("level_estimation", c.level), ("level_old", c.level_old), ("particle_size_class", c.size_class)):
            g.upload_field(f, v)
            o.upload_field(f, v)
    else:
        o = AC.upload(oracle_lib, c)
    for ctx in (g, o):
        ctx.set_split_patterns(SP.patterns if c.patterns else [])
    return g, o


def same_bits(g, o):
    assert g.n == o.n
    for f in AC.FIELDS:
        a, b = g.download(f), o.download(f)
        assert np.array_equal(a, b, equal_nan=f == "level_estimation"), (f, np.nonzero(np.reshape(a != b, (len(a), -1)).any(axis=1))[0][:8])


def steps_on(g, c, order="cold"):
    """after every successful apply: the lists belong to the state before it, and the edited vector steps"""
    if c.kind == "split" and c.note["extra"] == 0 and order == "permuted":
        g.download_neighbors()                                   # (a split with nobody TooLarge changes nothing: the step's lists still hold)
    else:
        with pytest.raises(ffi.SphError):
            g.download_neighbors()
    p = c.params().to_ffi()
    if g.n == 0:
        with pytest.raises(ffi.SphError) as e:                   # (the reference unwraps the maximum over no particles)
            g.step(p)
        assert e.value.status == 1
        return
    g.step(p)
    for f in ("position", "velocity", "density", "mass"):
        assert np.isfinite(g.download(f)).all(), f


@pytest.mark.parametrize("order", ["cold", "permuted"])
@pytest.mark.parametrize("c", APPLIED, ids=ids(APPLIED))
def test_apply_equals_the_oracle_bit_for_bit(product_lib, oracle_lib, c, order):
    g, o = pair(product_lib, oracle_lib, c, order)
    try:
        apply(g, c)
        apply(o, c)
        if c.kind == "merge":
            assert g.n == c.note["n_new"]
        if c.kind == "split":
            assert g.n == c.n + c.note["extra"]
        same_bits(g, o)
        steps_on(g, c, order)
    finally:
        g.close()
        o.close()


def test_merge_with_a_chunked_scan_carry(product_lib, oracle_lib):
    """n = 524 289 = 257 scan tiles: k_scan_sums carries from its first chunk of 256 tile sums into a second one.  One context, never stepped."""
    c = AC.merge_case_large()
    g, o = pair(product_lib, oracle_lib, c, "cold")
    try:
        apply(g, c)
        apply(o, c)
        assert g.n == c.note["n_new"]
        same_bits(g, o)
        with pytest.raises(ffi.SphError):
            g.download_neighbors()
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("order", ["cold", "permuted"])
@pytest.mark.parametrize("c", REFUSED, ids=ids(REFUSED))
def test_refused_split_leaves_every_field_as_it_was(product_lib, oracle_lib, c, order):
    """Compared by status only (the oracle's sequential split has split the parents in front of the one it panics at); on the product a
    refused call changes nothing."""
    g, o = pair(product_lib, oracle_lib, c, order)
    try:
        names = list(AC.FIELDS) + (["density", "pressure", "neighbor_count", "cell_index", "lambda_sum"] if order == "permuted" else [])
        before = {f: g.download(f) for f in names}
        status = []
        for ctx in (g, o):
            with pytest.raises(ffi.SphError) as e:
                apply(ctx, c)
            status.append(e.value.status)
        assert status == [c.status, c.status]
        assert g.n == c.n
        for f in names:
            assert np.array_equal(g.download(f), before[f], equal_nan=True), f
    finally:
        g.close()
        o.close()


# ---- the slab form -------------------------------------------------------------------------------------------------------------------
class SlabWorld:
    """A k-rank group of the slab scene that has stepped once, and what the case builders need from it: fields gathered by id, the rank of
    every id, the neighbour lists in global ids.  transport: loopback (sph_group_*) or threads (every rank calls from its own thread)."""

    def __init__(self, lib, k, interleaved, transport="loopback", capacities=None):
        self.pos, self.mass, self.vel, self.planes = AC.slab_scene(interleaved)
        self.k, self.thr = k, None
        self.cuts = D.slab_cuts(self.pos[:, 0], k)
        self.p = AC.dam_break_params(level_estimation_method="None").to_ffi()
        if transport == "threads":
            self.thr = D.ThreadedGroup(lib, self.pos, self.mass, self.vel, self.planes, k, capacities=capacities)
            self.ctxs = self.thr.contexts
        elif capacities is None:
            self.ctxs = D.make_loopback_group(lib, self.pos, self.mass, self.vel, self.planes, k)
        else:
            parts = D.partition(self.pos[:, 0], self.cuts)
            self.ctxs = []
            for r in range(k):
                ctx = ffi.Context(lib, capacities[r] or D._slab_capacity(len(self.mass), k), self.planes)
                ctx.dist_configure(r, k, self.cuts[r], self.cuts[r + 1])
                ctx.upload(self.mass[parts[r]], self.pos[parts[r]], self.vel[parts[r]])
                ctx.upload_field("particle_id", parts[r].astype(np.uint32))
                self.ctxs.append(ctx)
        for ctx in self.ctxs:
            ctx.set_split_patterns(SP.patterns)
        self.step()
        self.ids = [ctx.download("particle_id") for ctx in self.ctxs]
        self.n = int(sum(len(i) for i in self.ids))
        self.rank = AC.slab_rank_of(self.ids, self.n)
        off, self.idx = D.assemble_lists(self.ids, [ctx.download_neighbors() for ctx in self.ctxs], self.n)
        self.off = np.asarray(off, np.int64)
        self.f = {f: D.gather_by_id(self.ctxs, f, self.n) for f in ("mass", "position", "velocity", "h2", "h2_next")}

    def step(self):
        return self.thr.step(self.p) if self.thr else ffi.group_step(self.ctxs, self.p)

    def each_rank(self, fn):
        """fn(ctx) on every rank from its own thread -> the status of every rank (0: returned)"""
        futs = [self.thr.pool.submit(fn, ctx) for ctx in self.ctxs]
        out = []
        for fut in futs:
            try:
                fut.result()
                out.append(0)
            except ffi.SphError as e:
                out.append(e.status)
        return out

    def write(self, c):
        """the designed fields of the case to the ranks (rows of a rank: its owned particles in download order)"""
        for ctx, ids in zip(self.ctxs, self.ids):
            for f, v in (("mass", c.mass), ("level_estimation", c.level), ("level_old", c.level_old), ("particle_size_class", c.size_class)):
                ctx.upload_field(f, v[ids])

    def apply(self, c, p=None):
        """-> the ranks' statuses (loopback: the group call's status for all of them)"""
        p, ap = p or c.params().to_ffi(), c.adapt_params()
        if self.thr:
            if c.kind == "split":
                return self.each_rank(lambda ctx: ctx.split_particles(p, ap))
            return self.each_rank(lambda ctx: (ctx.share_particles if c.kind == "share" else ctx.merge_particles)(p, ap, c.merge_partner, c.merge_counter))
        try:
            ffi.group_adapt(self.ctxs, c.kind, p, ap, *(() if c.kind == "split" else (c.merge_partner, c.merge_counter)))
        except ffi.SphError as e:
            return [e.status] * self.k
        return [0] * self.k

    def close(self):
        if self.thr:
            self.thr.close()
        else:
            for ctx in self.ctxs:
                ctx.close()


def slab_specs(w, kind, n_parents=24):
    if kind == "transfer":
        return AC.slab_transfer_cases(w.n, w.rank, w.off, w.idx, w.f["mass"])
    return AC.slab_split_cases(w.n, w.rank, w.f["position"], w.f["mass"], w.cuts, n_parents)


def check_slab_case(w, oracle_lib, c):
    """the same global decisions on the group and on the oracle that holds the group's fields by id; every field by id, bit for bit"""
    (AC.check_slab_split_case if c.kind == "split" else AC.check_slab_transfer_case)(c, w.rank)
    o = ffi.Context(oracle_lib, c.capacity, w.planes)
    try:
        o.upload(c.mass, c.position, c.velocity)
        for f, v in c.fields().items():
            o.upload_field(f, v)
        o.set_split_patterns(SP.patterns)
        w.write(c)
        apply(o, c)
        assert w.apply(c) == [0] * w.k
        n = o.n
        assert sum(ctx.n for ctx in w.ctxs) == n
        got_ids = np.concatenate([ctx.download("particle_id") for ctx in w.ctxs])
        assert np.array_equal(np.sort(got_ids), np.arange(n))                              # the ids are the reference's indices 0 .. n'-1 again
        for f in AC.FIELDS:
            a, b = D.gather_by_id(w.ctxs, f, n), o.download(f)
            assert np.array_equal(a, b, equal_nan=f == "level_estimation"), (c.name, f, np.nonzero(np.reshape(a != b, (n, -1)).any(axis=1))[0][:8])
        if c.name.startswith("one rank is all"):
            assert w.ctxs[c.note["whole"]].n == 0                                           # a rank that lost every particle
        w.step()                                                                            # and the group steps with what the apply left it
        for f in ("position", "velocity", "density"):
            assert np.isfinite(D.gather_by_id(w.ctxs, f, n)).all(), f
    finally:
        o.close()


@pytest.mark.parametrize("case", range(5))
@pytest.mark.parametrize("k", [2, 3, 4])
def test_slab_transfers_equal_the_oracle_by_id(product_lib, oracle_lib, k, case):
    w = SlabWorld(product_lib, k, interleaved=False)
    try:
        specs = slab_specs(w, "transfer")
        assert len(specs) == 5
        check_slab_case(w, oracle_lib, AC.slab_case(specs[case], **w.f))
    finally:
        w.close()


@pytest.mark.parametrize("case", range(2))
@pytest.mark.parametrize("k", [2, 3, 4])
def test_slab_splits_equal_the_oracle_by_id(product_lib, oracle_lib, k, case):
    w = SlabWorld(product_lib, k, interleaved=True)
    try:
        check_slab_case(w, oracle_lib, AC.slab_case(slab_specs(w, "split")[case], **w.f))
    finally:
        w.close()


@pytest.mark.parametrize("what", ["straddling pairs", "alternating parents"])
def test_slab_apply_with_every_rank_on_its_own_thread(product_lib, oracle_lib, what):
    split = what == "alternating parents"
    w = SlabWorld(product_lib, 2, interleaved=split, transport="threads")
    try:
        check_slab_case(w, oracle_lib, AC.slab_case(slab_specs(w, "split" if split else "transfer")[0], **w.f))
    finally:
        w.close()


# ---- slab refusals: every rank leaves the call with a failure, nobody waits in a collective the refusing rank never enters ----------
def refusal_case(w, which):
    """-> (case, the rank that refuses, its status)"""
    n, rank = w.n, w.rank
    x = w.f["position"][:, 0]
    if which == "donor out of reach":
        # a receiver deep inside rank 0 whose donor lies deep inside rank 1: several support radii from the cut, so not among rank 0's ghosts
        r = int(np.nonzero(rank == 0)[0][np.argmin(x[rank == 0])])
        d = int(np.nonzero(rank == 1)[0][np.argmax(x[rank == 1])])
        assert x[d] - x[r] > 10 * w.f["h2_next"].max()
        partner, counter = np.full(n, AC.AV, np.uint32), np.zeros(n, np.uint16)
        partner[r], partner[d], counter[d] = d, AC.DEL, 1
        spec = dict(name=which, kind="merge", partner=partner, counter=counter, level=np.zeros(n, np.float32), overrides=AC.slab_overrides(np.median(w.f["mass"]) / 4), dt=0.001)
        return AC.slab_case(spec, **w.f), 0, 1                                              # SPH_ERR_INVALID_ARGUMENT
    spec = slab_specs(w, "split", 24 if which.startswith("1.49") else 120)[0]             # (capacity: more children than a ghost layer holds)
    c = AC.slab_case(spec, **w.f)
    if which == "1.4999999 on one rank":
        i = int(spec["parents"][rank[spec["parents"]] == 1][0])
        t = A.target_mass(c.level, c.params())[i]
        c.mass[i] = next(m for m in (AC.tie_mass(t, AC.JUST_BELOW), np.nextafter(np.float32(t) * np.float32(1.25), np.float32(0))) if m is not None)
        assert AC.num_children(c.mass[i], t, 59, False) is None
        return c, 1, 27
    return c, 1, 3                                                                          # "capacity one short on one rank"


def children_on(c, rank, r):
    t = A.target_mass(c.level, c.params())
    return sum(AC.num_children(c.mass[i], t[i], 59, False) - 1 for i in c.note["parents"] if rank[i] == r)


@pytest.mark.parametrize("transport", ["loopback", "threads"])
@pytest.mark.parametrize("which", ["donor out of reach", "1.4999999 on one rank", "capacity one short on one rank"])
def test_slab_refusals_end_on_all_ranks_together(product_lib, which, transport):
    """Modelled on test_gpu_slabs.py::test_ranks_on_threads_capacity_failure_is_collective: a refusal on ONE rank is that rank's status
    in each_member and agree() ends the call on every rank.  Nothing is asserted about the fields afterwards (slab_adapt: the records
    were written)."""
    k = 2
    capacities = None
    if which.startswith("capacity"):
        probe = SlabWorld(product_lib, k, interleaved=True)                                  # the same world: what rank 1 owns, what its parents need
        try:
            c, r, _ = refusal_case(probe, which)
            n_own, kids = probe.ctxs[r].n, children_on(c, probe.rank, r)
            ghosts = sum(probe.ctxs[r].dist_get_stats()["n_ghost"])
        finally:
            probe.close()
        assert kids > 2 * ghosts + 64                                                        # the step fits into a capacity that the split misses by one
        capacities = [None] * k
        capacities[r] = n_own + kids - 1
    w = SlabWorld(product_lib, k, interleaved=which != "donor out of reach", transport=transport, capacities=capacities)
    try:
        c, r, status = refusal_case(w, which)
        if capacities:
            assert w.ctxs[r].n + children_on(c, w.rank, r) == capacities[r] + 1
        w.write(c)
        got = w.apply(c)
        assert got[r] == status and all(s != 0 for s in got), got
    finally:
        w.close()
