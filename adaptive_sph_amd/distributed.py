"""Slab decomposition glue: one process per GPU (torch.distributed is plumbing only -- it carries the RCCL
unique id and the launcher's barrier; the halo exchange itself is RCCL inside libsph_hip.so).

  slab_cuts          x-cuts that give every rank the same number of particles (quantiles of x)
  partition          indices of the particles each rank owns
  make_slab_context  context of this rank, configured, communicator initialised, particles uploaded
  make_loopback_group  k contexts in this process (ranks 0..k-1) for single-GPU verification
  group_single_step_adaptivity  single_step_adaptivity for a slab group, through a gather to one context and back
  rank_single_step_adaptivity   the same with one process per rank: gather / scatter through the launcher's process group
  rank_single_step_adaptivity_on_slabs         the particles stay on their ranks; the decisions on the root's host, through the launcher
  rank_single_step_adaptivity_on_slabs_device  ... the decisions on the root's device, relayed over the ranks' own transport
  ThreadedGroup      k ranks of this process, one host thread each, every rank calling sph_step by itself (verification of the per-rank code)
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from . import ffi

INF = float(np.finfo(np.float32).max)


def slab_cuts(x: np.ndarray, n_ranks: int) -> List[float]:
    """n_ranks+1 cut positions: -inf, quantiles of x, +inf.  Rank r owns cut[r] <= x < cut[r+1]."""
    xs = np.sort(np.asarray(x, dtype=np.float32))
    cuts = [-INF]
    for r in range(1, n_ranks):
        k = (len(xs) * r) // n_ranks
        # cut half-way between two distinct x values so that equal coordinates stay on one side
        lo = xs[max(k - 1, 0)]
        hi = xs[min(k, len(xs) - 1)]
        cuts.append(float(np.float32((np.float64(lo) + np.float64(hi)) * 0.5)) if hi > lo else float(hi))
    cuts.append(INF)
    return cuts


def partition(x: np.ndarray, cuts: Sequence[float]) -> List[np.ndarray]:
    x = np.asarray(x, dtype=np.float32)
    out = []
    for r in range(len(cuts) - 1):
        lo, hi = np.float32(cuts[r]), np.float32(cuts[r + 1])
        out.append(np.nonzero((x >= lo) & (x < hi))[0] if r + 1 < len(cuts) - 1 else np.nonzero(x >= lo)[0])
    return out


def _slab_capacity(n_total: int, n_ranks: int) -> int:
    # room for imbalance as the fluid moves (static cuts) plus the ghost layers
    return int(n_total / n_ranks * 2.5) + 65536


def pick_transport(world: int) -> str:
    """"rccl" -- one rank per GPU over xGMI, the fast path -- unless the launch puts several ranks on one device (RCCL refuses that:
    "Duplicate GPU detected") or SPH_TRANSPORT=shm asks for the host-staged shared-memory transport (sph_comm_init_shm)."""
    import os
    import torch
    want = os.environ.get("SPH_TRANSPORT", "")
    if want in ("shm", "rccl", "ipc"):   # ipc: the peer-mapped push transport (device to device, no RCCL launch per exchange) on top of shm
        return want
    return "shm" if (torch.cuda.is_available() and world > torch.cuda.device_count()) else "rccl"


_SHM_SERIAL = [0]


def make_slab_context(lib: ffi.SphLibrary, pos, mass, vel, planes, rank: int, world: int, local_rank: int, transport: str = None,
                      cuts: Sequence[float] = None, bytes_per_side: int = None) -> ffi.Context:
    """This rank's slab context of a `torch.distributed` launch (one process per rank): configured, communicator attached, particles
    uploaded.  torch.distributed only carries the RCCL unique id (or the shared-memory segment's name) and a barrier.  `cuts`: the
    world + 1 static cuts (default: slab_cuts, equal counts).  `bytes_per_side` (shared-memory and peer-mapped transports): the size of an
    outbox / inbox, the most one message may hold (default: room for every particle of the slab as a migrant record)."""
    import os
    import torch.distributed as dist
    import torch
    transport = transport or pick_transport(world)
    cuts = list(cuts) if cuts is not None else slab_cuts(pos[:, 0], world)
    mine = partition(pos[:, 0], cuts)[rank]
    cap = _slab_capacity(len(mass), world)
    ctx = ffi.Context(lib, cap, planes, device_id=local_rank)
    ctx.dist_configure(rank, world, cuts[rank], cuts[rank + 1])
    ctx.upload(mass[mine], pos[mine], vel[mine])
    if world > 1:
        ctx.upload_field("particle_id", mine.astype(np.uint32))
    if transport in ("shm", "ipc"):
        # rank 0 names and creates the segment, the others map it after the launcher's barrier; an outbox holds one message to one
        # x-neighbour: at most every particle of the slab as a 48-byte migrant record
        _SHM_SERIAL[0] += 1
        name = [f"/sph_shm_{os.getpid()}_{_SHM_SERIAL[0]}" if rank == 0 else None]
        dist.broadcast_object_list(name, src=0)
        per_side = int(bytes_per_side) if bytes_per_side else max(1 << 22, cap * 48)
        if rank == 0:
            ctx.comm_init_shm(name[0], rank, world, per_side, True)
        dist.barrier()
        if rank != 0:
            ctx.comm_init_shm(name[0], rank, world, per_side, False)
        dist.barrier()
        if transport == "ipc":
            # every rank exports its device inbox, the launcher all-gathers the 64-byte handles, every rank maps the others'.  A rank
            # whose export or mapping fails tells the others THROUGH the gather (None / a flag) instead of leaving them in it: every rank
            # then raises the same error
            try:
                mine_h, err = ctx.comm_ipc_export(per_side), None
            except ffi.SphError as e:
                mine_h, err = None, str(e)
            handles = [None] * world
            dist.all_gather_object(handles, (mine_h, err))
            bad = [(r, h[1]) for r, h in enumerate(handles) if h[0] is None]
            if bad:
                raise ffi.SphError(2, f"peer-mapped transport: rank {bad[0][0]} could not export its inbox: {bad[0][1]}")
            try:
                ctx.comm_init_ipc(b"".join(h[0] for h in handles), world)
                err = None
            except ffi.SphError as e:
                err = str(e)
            errs = [None] * world
            dist.all_gather_object(errs, err)
            bad = [(r, e) for r, e in enumerate(errs) if e]
            if bad:
                raise ffi.SphError(2, f"peer-mapped transport: rank {bad[0][0]} could not map its peers' inboxes: {bad[0][1]}")
        return ctx
    # RCCL unique id: created on rank 0, broadcast through the launcher's process group
    buf = torch.zeros(128, dtype=torch.uint8)
    if rank == 0:
        import ctypes as C
        raw = (C.c_uint8 * 128)()
        rc = lib.comm_unique_id(raw)
        if rc != 0:
            raise ffi.SphError(rc, "ncclGetUniqueId failed")
        buf = torch.tensor(list(raw), dtype=torch.uint8)
    dev = torch.device("cuda", local_rank) if dist.get_backend() == "nccl" else torch.device("cpu")
    buf = buf.to(dev)
    dist.broadcast(buf, src=0)
    ctx.comm_init(bytes(buf.cpu().numpy().tolist()), rank, world)
    return ctx


def make_loopback_group(lib: ffi.SphLibrary, pos, mass, vel, planes, n_ranks: int, device_id: int = 0, cuts: Sequence[float] = None) -> List[ffi.Context]:
    cuts = list(cuts) if cuts is not None else slab_cuts(pos[:, 0], n_ranks)
    parts = partition(pos[:, 0], cuts)
    ctxs = []
    for r in range(n_ranks):
        c = ffi.Context(lib, _slab_capacity(len(mass), n_ranks), planes, device_id=device_id)
        c.dist_configure(r, n_ranks, cuts[r], cuts[r + 1])
        c.upload(mass[parts[r]], pos[parts[r]], vel[parts[r]])
        c.upload_field("particle_id", parts[r].astype(np.uint32))
        ctxs.append(c)
    return ctxs


def gather_by_id(contexts: Sequence[ffi.Context], name: str, n_total: int) -> np.ndarray:
    """Reassemble a field of all ranks into global particle order (loopback / rank-0 diagnostics)."""
    fid, dt, w = ffi.FIELDS[name]
    out = np.zeros((n_total, w) if w > 1 else (n_total,), dtype=dt)
    for c in contexts:
        ids = c.download("particle_id")
        out[ids] = c.download(name)
    return out


_ADAPT_FIELDS = ("h2", "h2_next", "level_estimation", "level_old", "particle_size_class")


def assemble_lists(ids: Sequence[np.ndarray], lists: Sequence, n: int):
    """The ranks' exported neighbour lists -- rank r: rows of its owned particles in the order of ids[r], (offsets, indices) with
    global ids as indices -- as ONE CSR in global index order: row i = the list of the particle with id i."""
    counts = np.zeros(n, np.int64)
    for i, (off, _) in zip(ids, lists):
        counts[np.asarray(i, np.int64)] = np.diff(np.asarray(off, np.int64))
    off_g = np.zeros(n + 1, np.int64)
    np.cumsum(counts, out=off_g[1:])
    idx_g = np.empty(int(off_g[-1]), np.uint32)
    for i, (off, idx) in zip(ids, lists):
        off = np.asarray(off, np.int64)
        lens = np.diff(off)
        # entry e of this rank's index array sits in row r(e); its place in the global CSR = start of that row's global row + (e - off[r])
        dst = np.repeat(off_g[np.asarray(i, np.int64)] - off[:-1], lens) + np.arange(len(idx))
        idx_g[dst] = idx
    return off_g, idx_g


_PROBLEM_FIELDS = ("particle_size_class", "mass", "level_estimation", "position", "h2")


def merge_slab_partner_problems(parts: Sequence[dict], dense: bool = None):
    """The ranks' local partner problems (Context.slab_partner_problem_download, one dict per rank: "ids" with the "n_owned" owned
    participants first, the five decision fields at ids, "offsets"[n_owned + 1] / "indices": the owned participants' candidate rows in
    global ids) as ONE problem of size K, in the layout of adaptivity.partner_problem_reference -- which it equals, array for array, on
    the gathered fields and the assembled full lists: (ids, size_class, mass, level, position, h2, offsets, indices) with ids the
    union of the ranks' ids in ascending order, the fields from whichever rank holds the particle, the rows of the owned participants
    relabelled to compact ids and an empty row for a participant that is nobody's donor.  Pure numpy.

    A particle two ranks report (owned on one and a ghost on another, or a ghost on two) must come with the same bits from both: the
    ghost records are refreshed from the owner inside the prepare.  Different values raise ValueError -- picking one would hide a stale
    ghost.  So does a particle two ranks claim to own, and an entry that names no participant.

    `dense`: how an id finds its compact id.  True: through a table over 0 .. the largest id (one host word per id below it, no sort
    and no binary search: at K near n, 4 M participants and 32 M entries, the sorted form took 1.6 s of a 1.6 s pass).  False: sort
    (np.unique) and np.searchsorted, whose memory follows the problem and not the ids.  None: the table while the largest id is below
    8 x (participants + entries reported)."""
    ids_all = [np.asarray(q["ids"], np.uint32) for q in parts]
    reported = int(sum(len(i) for i in ids_all)) + int(sum(len(q["indices"]) for q in parts))
    top = max([int(i.max()) for i in ids_all if len(i)], default=-1)
    if dense is None:
        dense = top < 8 * reported
    if dense:
        flag = np.zeros(top + 1, bool)
        for i in ids_all:
            flag[i] = True
        ids = np.flatnonzero(flag).astype(np.uint32)
        K = len(ids)
        table = np.empty(top + 1, np.int64)
        table[ids] = np.arange(K, dtype=np.int64)
        where = [table[i] for i in ids_all]

        def compact_of(idx):
            """-> (compact ids, every entry names a participant)"""
            inside = idx <= top if len(idx) else np.ones(0, bool)
            ok = bool(np.all(inside)) and bool(np.all(flag[idx]))
            return (table[idx] if ok else np.zeros(len(idx), np.int64)), ok
    else:
        ids = np.unique(np.concatenate(ids_all + [np.empty(0, np.uint32)])).astype(np.uint32)
        K = len(ids)
        where = [np.searchsorted(ids, i) for i in ids_all]

        def compact_of(idx):
            c = np.searchsorted(ids, idx)
            return c, not len(idx) or bool(np.all(c < K) and np.array_equal(ids[np.minimum(c, K - 1)], idx))
    fields = []
    for f in _PROBLEM_FIELDS:
        first = np.asarray(parts[0][f])
        tail = first.shape[1:]
        width = int(np.prod(tail, dtype=np.int64)) * first.dtype.itemsize   # bytes per participant
        out = np.zeros((K,) + tail, first.dtype)
        seen = np.zeros(K, bool)
        for q, w in zip(parts, where):
            v = np.ascontiguousarray(q[f], first.dtype).reshape((len(w),) + tail)
            again = seen[w]
            a = np.ascontiguousarray(out[w[again]]).view(np.uint8).reshape(-1, width)
            b = np.ascontiguousarray(v[again]).view(np.uint8).reshape(-1, width)
            if not np.array_equal(a, b):
                bad = ids[w[again]][np.any(a != b, axis=1)]
                raise ValueError(f"merge_slab_partner_problems: particle {int(bad[0])} comes with different {f} from two ranks ({len(bad)} such particles)")
            out[w] = v
            seen[w] = True
        fields.append(out)
    owner = np.full(K, -1, np.int64)
    rows, lists = [], []
    for r, (q, w) in enumerate(zip(parts, where)):
        ko = int(q["n_owned"])
        mine = w[:ko]
        if (owner[mine] >= 0).any():
            raise ValueError(f"merge_slab_partner_problems: particle {int(ids[mine[owner[mine] >= 0][0]])} is owned by two ranks")
        owner[mine] = r
        idx = np.asarray(q["indices"], np.uint32)
        c, known = compact_of(idx)
        if not known:
            raise ValueError(f"merge_slab_partner_problems: rank {r} has a candidate that is no participant")
        off = np.asarray(q["offsets"], np.int64)
        if len(off) != ko + 1 or int(off[-1]) != len(idx):
            raise ValueError(f"merge_slab_partner_problems: rank {r}: {len(off)} offsets for {ko} owned participants, {len(idx)} entries")
        rows.append(mine)
        lists.append((off, c.astype(np.uint32)))
    off_c, idx_c = assemble_lists(rows, lists, K)
    return (ids, *fields, off_c.astype(np.uint32), idx_c)


class GatherContext:
    """The ONE plain context an adaptive step of a slab decomposition runs on (the reference decides sequentially over ALL particles
    in index order, and a transfer's two partners may sit on different ranks: exactness goes through one place).  Kept between
    adaptive steps -- allocating and freeing every per-particle buffer each time costs more than the step -- on the device the
    caller names.  MEMORY: the whole particle set of the decomposition must fit that ONE device next to the rank's own slab
    (~290 B per particle of capacity): scenes that need slabs to fit at all cannot take this path."""

    def __init__(self, lib: ffi.SphLibrary, planes, device_id: int = 0, split_patterns=None, log=None):
        self.lib, self.planes, self.device_id, self.split_patterns, self.log = lib, planes, device_id, split_patterns, log
        self.ctx = None
        self.driver = None

    def ensure(self, n: int, capacity: int = 0):
        from .adaptivity import AdaptivityDriver
        want = capacity or max(2 * n, n + 65536)
        if self.ctx is None or self.ctx.capacity < want:
            self.close()
            self.ctx = ffi.Context(self.lib, want, self.planes, device_id=self.device_id)
            self.driver = AdaptivityDriver(self.ctx, self.split_patterns, self.log)
        return self.ctx

    def close(self):
        if self.ctx is not None:
            self.ctx.close()
        self.ctx, self.driver = None, None


def _adapt_gathered(gc: GatherContext, P, dt: float, step_number: int, g: dict, ids: Sequence[np.ndarray], lists: Sequence, capacity: int = 0):
    """`g`: the fields of ALL particles in global index order; `ids` / `lists`: the ranks' ids and exported neighbour lists.
    -> (fields of the new vector in its index order, info)."""
    n = len(g["mass"])
    off_g, idx_g = assemble_lists(ids, lists, n)   # neighbour lists in index order
    if off_g[-1] >= 2 ** 32:
        raise ValueError(f"adaptive step of a slab decomposition: {int(off_g[-1])} neighbour-list entries do not fit the 32-bit CSR offsets of the partner search")
    T = gc.ensure(n, capacity)
    T.upload(g["mass"], g["position"], g["velocity"])
    for f in _ADAPT_FIELDS:
        T.upload_field(f, g[f])
    info = gc.driver.single_step_adaptivity(P, dt, step_number, lists=(off_g.astype(np.uint32), idx_g))
    new = {f: T.download(f) for f in ("mass", "position", "velocity") + _ADAPT_FIELDS}
    info["n_after"] = len(new["mass"])
    return new, info


def _reupload(c: ffi.Context, new: dict, mine: np.ndarray):
    c.upload(new["mass"][mine], new["position"][mine], new["velocity"][mine])
    for f in _ADAPT_FIELDS:
        c.upload_field(f, new[f][mine])
    c.upload_field("particle_id", mine.astype(np.uint32))


def group_single_step_adaptivity(lib: ffi.SphLibrary, contexts: Sequence[ffi.Context], planes, P, dt: float, step_number: int,
                                 split_patterns=None, capacity: int = 0, log=None, gather: GatherContext = None) -> dict:
    """single_step_adaptivity (simulation.rs:2732-2796) for the ranks of a slab decomposition that have just stepped.

    The reference decides sequentially over ALL particles in index order and a transfer's two partners may sit on different
    ranks, so the exact form goes through one place: the owned particles of every rank (mass, position, velocity, h2, h2_next,
    level values, size class) and their neighbour lists (global ids, ghosts included) are assembled in global index order -- the
    particle ids ARE the reference's Vec indices --, uploaded to ONE plain context (GatherContext: pass one to keep it between
    steps), the same decisions (adaptivity.py) and the same device-side share / merge / split run there, and the result goes
    back: every rank is re-uploaded with the particles of its slab, their new index as id.  Same arithmetic as on a single
    context; the price is a gather and a scatter over PCIe per adaptive step (support lengths FromMass: the previous step's lambda
    sums do not travel).  In-process form (loopback group, or one process driving several GPUs); rank_single_step_adaptivity is
    the same for one process per GPU."""
    if P.support_length_estimation != "FromMass":
        raise ValueError("group_single_step_adaptivity: support_length_estimation must be FromMass")
    ids = [c.download("particle_id") for c in contexts]
    n = int(sum(len(i) for i in ids))
    allid = np.concatenate(ids)
    if not np.array_equal(np.sort(allid), np.arange(n, dtype=allid.dtype)):
        raise ValueError("group_single_step_adaptivity: the particle ids of the ranks are not the indices 0 .. n-1")
    g = {f: gather_by_id(contexts, f, n) for f in ("mass", "position", "velocity") + _ADAPT_FIELDS}
    own = gather is None
    gc = gather or GatherContext(lib, planes, 0, split_patterns, log)
    try:
        new, info = _adapt_gathered(gc, P, dt, step_number, g, ids, [c.download_neighbors() for c in contexts], capacity)
    finally:
        if own:
            gc.close()
    cuts = [contexts[0].dist_get_cuts()[0]] + [c.dist_get_cuts()[1] for c in contexts]
    parts = partition(new["position"][:, 0], [-INF] + [float(v) for v in cuts[1:-1]] + [INF])
    for c, mine in zip(contexts, parts):
        _reupload(c, new, mine)
    return info


C_INFO_BYTES = 48   # sizeof(sph_partner_search_info): what one device search brings down
SLAB_EXPORTS = ("lists", "candidates", "compact")
GROUP_SLAB_EXPORTS = SLAB_EXPORTS + ("device",)   # the in-process group form also solves on the device (include/sph_slab_partner_search.h)


def _decide_compact(lib, kind: str, ids, fields, off_c, idx_c, P, dt: float):
    """the same search on the merged compact problem (n = K): -> (partner_c, counter_c) in compact ids"""
    from .adaptivity import find_partners_native
    return find_partners_native(lib, kind, *fields, off_c, idx_c, P, dt)


def _count_slab_problem(info: dict, kind: str, K: int, counts, ranks_up: int):
    """what one compact pass moves: `counts` the (participants, owned participants, candidates) of the ranks whose problems came down
    HERE, `ranks_up` how many ranks take the K decisions from here"""
    info["participants"] += K
    info["exported_indices"] += int(sum(t for _, _, t in counts))
    info["bytes_down"] += int(sum(25 * k + 4 * (ko + 1) + 4 * t for k, ko, t in counts))
    info["bytes_up"] += 10 * K * ranks_up
    info["passes"].append({"kind": kind, "participants": K, "ranks": [tuple(int(v) for v in c) for c in counts]})


def _decide_on_gathered(lib, kind: str, g: dict, lists, P, dt: float):
    """find_share_partner_sequential / find_merge_partner_sequential over the WHOLE vector (fields in global index order)"""
    from .adaptivity import find_partners_native
    return find_partners_native(lib, kind, g["particle_size_class"], g["mass"], g["level_estimation"], g["position"], g["h2"], lists[0], lists[1], P, dt)


def group_single_step_adaptivity_on_slabs(lib: ffi.SphLibrary, contexts: Sequence[ffi.Context], P, dt: float, step_number: int, log=None,
                                          export: str = "lists") -> dict:
    """single_step_adaptivity (simulation.rs:2732-2796) for the ranks of a slab group that have just stepped, WITHOUT moving the
    particles: the DECISIONS are taken where the reference takes them -- sequentially over the whole vector, here on the host over
    the fields the searches read (size class, mass, level, position, h2: 21 B per particle) and the step's neighbour lists, gathered
    by global id -- and applied by every rank to its own slab (sph_group_adapt: the slab form of share / merge / split).  Same
    arithmetic, same indices as on one context; nothing is re-uploaded.  (Every context needs its split patterns:
    Context.set_split_patterns.)

    `export`: "lists" -- every rank exports its whole CSR (sph_download_neighbors), assembled once and kept across the passes -- or
    "candidates": before each search every rank filters its donors' rows on the device (sph_group_slab_candidates_prepare,
    include/sph_slab_candidates.h) and exports only the entries that pass the search's class and distance tests; the same search runs
    on the assembled candidate rows and takes the same decisions.  No sph_download_neighbors in that mode, and the mass check adds
    the ranks' device sums (sph_slab_sum_mass).  info["export"], ["exported_indices"], ["bytes_down"] count what came down as
    AdaptivityDriver counts it (4 B per index, offset and id, 21 B per particle for the five fields, 4 B per downloaded mass, 8 B per
    device sum).

    "compact" (include/sph_slab_partner_problem.h): before each search every rank packs its LOCAL problem on the device
    (sph_group_slab_partner_problem_prepare: the same rows, then only the particles they touch), the ranks' problems are merged by id
    into one problem of K participants (merge_slab_partner_problems), the same search runs with n = K and every rank takes the K
    decisions (sph_group_adapt_compact).  No particle ids, no field of the whole vector and no list comes down.  info["participants"]:
    the sum of K over the passes; ["bytes_down"]: 25 B per local participant (id, class, mass, level, position, h2), 4 B per offset of
    an owned participant's row (one more than there are), 4 B per candidate, 8 B per device sum; ["bytes_up"] (compact only): 10 B x K
    per rank; ["passes"]: per search its kind, K and the ranks' (participants, owned participants, candidates).

    "device" (include/sph_slab_partner_search.h; this in-process form only): the local problems are packed as for "compact", merged on
    member 0's device, solved there in the search's exact parallel schedule and validated, the K decisions go to every member device
    to device and every member applies its copy (sph_group_find_partners_device, sph_group_adapt_device): the same decisions, the
    same state.  No problem comes down and no decision goes up: ["bytes_down"] counts the 48 B info struct per search and the 8 B
    device sums, ["bytes_up"] is 0, ["bytes_between_devices"] what the members' buffers exchange with the root's -- 25 B per local
    participant, 4 B per offset and per candidate towards the root, 10 B x K back to every member, the root's own copies not counted;
    ["passes"]: per search its kind, K ("participants"), the ranks' local counts ("ranks"), rounds, max_frontier and wide_rounds."""
    from .adaptivity import adapt_params
    if P.support_length_estimation != "FromMass":
        raise ValueError("group_single_step_adaptivity_on_slabs: support_length_estimation must be FromMass")
    if export not in GROUP_SLAB_EXPORTS:
        raise ValueError(f"group_single_step_adaptivity_on_slabs: export must be one of {GROUP_SLAB_EXPORTS}, not {export!r}")
    device = export == "device"
    compact = export == "compact" or device   # (what the two share: no ids, no whole field, the device mass sums)
    candidates = export == "candidates"
    p, ap = P.to_ffi(), adapt_params(P, dt)
    ids = None if compact else [c.download("particle_id") for c in contexts]
    n = int(sum(c.n for c in contexts))
    info = {"n_before": n, "shares": 0, "merges": 0, "splits": 0, "export": export, "exported_indices": 0, "bytes_down": 0 if compact else 4 * n}
    if compact:
        info.update(participants=0, bytes_up=0, passes=[])
    if device:
        info["bytes_between_devices"] = 0
    lists = None

    def mass_sum():
        if candidates or compact:
            info["bytes_down"] += 8 * len(contexts)
            return float(sum(c.slab_sum_mass() for c in contexts))
        info["bytes_down"] += 4 * int(sum(c.n for c in contexts))
        return float(sum(c.download("mass").sum(dtype=np.float64) for c in contexts))

    if not candidates and not compact:
        off_g, idx_g = assemble_lists(ids, [c.download_neighbors() for c in contexts], n)   # the step's lists, kept across the passes like self.neighs
        if off_g[-1] >= 2 ** 32:
            raise ValueError(f"adaptive step of a slab decomposition: {int(off_g[-1])} neighbour-list entries do not fit the 32-bit CSR offsets of the partner search")
        lists = (off_g.astype(np.uint32), idx_g)
        info["exported_indices"] += len(idx_g)
        info["bytes_down"] += 4 * (n + len(contexts) + len(idx_g))
    total_mass1 = mass_sum()

    def gathered():
        for c in contexts:
            c.classify(p)
        info["bytes_down"] += 21 * n
        return {f: gather_by_id(contexts, f, n) for f in ("particle_size_class", "mass", "level_estimation", "position", "h2")}

    def decide(kind):
        g = gathered()
        if not candidates:
            return _decide_on_gathered(lib, kind, g, lists, P, dt)
        # this search's rows: the step's lists (kept on the ranks across the share), the fields as they are now
        ffi.group_slab_candidates_prepare(contexts, kind, p, ap)
        off_c, idx_c = assemble_lists(ids, [c.slab_candidates_download() for c in contexts], n)
        info["exported_indices"] += len(idx_c)
        info["bytes_down"] += 4 * (n + len(contexts) + len(idx_c))
        return _decide_on_gathered(lib, kind, g, (off_c.astype(np.uint32), idx_c), P, dt)

    def search(kind):
        """-> (the transfers decided, the apply of those decisions)"""
        if not compact:
            mp, mc = decide(kind)
            return int(mc.sum()), lambda: ffi.group_adapt(contexts, kind, p, ap, mp, mc)
        for c in contexts:
            c.classify(p)
        if device:
            root = 0
            found = ffi.group_find_partners_device(contexts, kind, p, ap, root=root)
            K, counts = found["participants"], found["ranks"]
            info["participants"] += K
            info["exported_indices"] += int(sum(t for _, _, t in counts))
            info["bytes_down"] += C_INFO_BYTES
            info["bytes_between_devices"] += int(sum(25 * k + 4 * (ko + 1) + 4 * t for r, (k, ko, t) in enumerate(counts) if r != root and k)) + 10 * K * (len(contexts) - 1)
            info["passes"].append({"kind": kind, "participants": K, "ranks": counts, "rounds": found["rounds"], "max_frontier": found["max_frontier"],
                                   "wide_rounds": found["wide_rounds"]})
            return found["transfers"], lambda: ffi.group_adapt_device(contexts, kind, p, ap)
        counts = ffi.group_slab_partner_problem_prepare(contexts, kind, p, ap)
        parts = [c.slab_partner_problem_download() for c in contexts]
        pids, *fields, off_c, idx_c = merge_slab_partner_problems(parts)
        _count_slab_problem(info, kind, len(pids), counts, len(contexts))
        mp_c, mc_c = _decide_compact(lib, kind, pids, fields, off_c, idx_c, P, dt)
        return int(mc_c.sum()), lambda: ffi.group_adapt_compact(contexts, kind, p, ap, pids, mp_c, mc_c)

    if P.sharing:
        info["shares"], apply = search("share")
        if log:
            log(f"SEQUENTIAL SHARE {info['shares']} shares")
        apply()
    if step_number % 2 == 0:
        if P.merging:
            info["merges"], apply = search("merge")
            if log:
                log(f"SEQUENTIAL MERGE {info['merges']} merges")
            apply()
    elif P.splitting:
        for c in contexts:
            c.classify(p)
        ffi.group_adapt(contexts, "split", p, ap)
        info["splits"] = int(sum(c.n for c in contexts)) - n
    total_mass2 = mass_sum()
    if not abs(total_mass1 - total_mass2) <= 0.005:             # assert_ft_approx_eq(total_mass1, total_mass2, 0.005, "mass sum"), in f64 (adaptivity.py)
        raise AssertionError(f"mass sum: {total_mass1} vs {total_mass2}")
    info["n_after"] = int(sum(c.n for c in contexts))
    return info


def rank_single_step_adaptivity_on_slabs(ctx: ffi.Context, P, dt: float, step_number: int, root: int = 0, export: str = "lists") -> dict:
    """The same with ONE PROCESS PER RANK (the RCCL / shared-memory / thread transports): every rank sends `root` the fields the
    partner searches read and its exported neighbour lists through the launcher's process group, `root` decides over the whole
    vector and broadcasts merge_partner / merge_counter (6 B per particle), every rank applies them to its own slab (the slab form
    of sph_share_particles / sph_merge_particles / sph_split_particles: collective calls through the context's own transport).
    Every rank calls this after the same sph_step; a failure on the root is re-raised on every rank.  `export`: as in
    group_single_step_adaptivity_on_slabs -- with "candidates" every rank prepares (sph_slab_candidates_prepare: collective through the
    context's transport) and sends the root its candidate rows before each search instead of its whole CSR once; the counts in info
    are this rank's.  With "compact" every rank prepares and sends the root its LOCAL problem (sph_slab_partner_problem_prepare:
    collective), the root merges them (merge_slab_partner_problems), decides on the K participants and broadcasts (ids, partner_c,
    counter_c) -- 10 B per participant instead of 6 B per particle --, and every rank applies them (sph_slab_share_particles_compact /
    sph_slab_merge_particles_compact); no particle id, no whole field and no list leaves the device."""
    import torch.distributed as dist
    from .adaptivity import adapt_params
    if P.support_length_estimation != "FromMass":
        raise ValueError("rank_single_step_adaptivity_on_slabs: support_length_estimation must be FromMass")
    if export == "device":
        raise ValueError("rank_single_step_adaptivity_on_slabs: export=\"device\" exists for the in-process group form only (group_single_step_adaptivity_on_slabs: "
                         "the transports between processes have no gather to a root; rank_single_step_adaptivity_on_slabs_device relays over the rank's own transport)")
    if export not in SLAB_EXPORTS:
        raise ValueError(f"rank_single_step_adaptivity_on_slabs: export must be one of {SLAB_EXPORTS}, not {export!r}")
    candidates = export == "candidates"
    compact = export == "compact"
    import time
    rank, world = dist.get_rank(), dist.get_world_size()
    p, ap = P.to_ffi(), adapt_params(P, dt)
    count = {"exported_indices": 0, "bytes_down": 0}
    if compact:
        count.update(participants=0, bytes_up=0, passes=[])
    # where the adaptive step's time goes (this rank's clock): device -> host (lists, fields), the launcher's
    # gather / broadcast (pickled numpy arrays), the host's partner search on the root, the apply calls on the slabs
    tm = {"download_s": 0.0, "gather_broadcast_s": 0.0, "host_decide_s": 0.0, "apply_s": 0.0}
    t0 = time.perf_counter()
    lists_mine = None if candidates or compact else ctx.download_neighbors()
    ids_mine = None if compact else ctx.download("particle_id")
    tm["download_s"] += time.perf_counter() - t0
    count["bytes_down"] += 0 if compact else 4 * len(ids_mine)
    if not candidates and not compact:
        count["exported_indices"] += len(lists_mine[1])
        count["bytes_down"] += 4 * (len(lists_mine[0]) + len(lists_mine[1]))
    state = {"lists": None, "n": 0}

    def decide(kind):
        """-> (merge_partner, merge_counter) of the whole vector on every rank"""
        t0 = time.perf_counter()
        ctx.classify(p)
        mine = {f: ctx.download(f) for f in ("particle_size_class", "mass", "level_estimation", "position", "h2")}
        count["bytes_down"] += 21 * len(ids_mine)
        if candidates:   # this search's rows, filtered where the lists are (every rank enters the prepare: it is collective)
            ctx.slab_candidates_prepare(kind, p, ap)
            mine["lists"] = ctx.slab_candidates_download()
            state["lists"] = None
            count["exported_indices"] += len(mine["lists"][1])
            count["bytes_down"] += 4 * (len(mine["lists"][0]) + len(mine["lists"][1]))
        tm["download_s"] += time.perf_counter() - t0
        mine["particle_id"] = ids_mine
        if state["lists"] is None and not candidates:
            mine["lists"] = lists_mine
        parts = [None] * world if rank == root else None
        t0 = time.perf_counter()
        dist.gather_object(mine, parts, dst=root)
        tm["gather_broadcast_s"] += time.perf_counter() - t0
        out = [None]
        t0 = time.perf_counter()
        if rank == root:
            try:
                n = int(sum(len(q["particle_id"]) for q in parts))
                if state["lists"] is None:
                    off_g, idx_g = assemble_lists([q["particle_id"] for q in parts], [q["lists"] for q in parts], n)
                    if off_g[-1] >= 2 ** 32:
                        raise ValueError(f"{int(off_g[-1])} neighbour-list entries do not fit the 32-bit CSR offsets of the partner search")
                    state["lists"] = (off_g.astype(np.uint32), idx_g)
                g = {}
                for f in ("particle_size_class", "mass", "level_estimation", "position", "h2"):
                    a = np.zeros((n,) + parts[0][f].shape[1:], parts[0][f].dtype)
                    for q in parts:
                        a[q["particle_id"]] = q[f]
                    g[f] = a
                out = [_decide_on_gathered(ctx.lib, kind, g, state["lists"], P, dt)]
            except Exception as e:  # noqa: BLE001 -- re-raised on every rank below
                out = [(None, (type(e).__name__, e.status if isinstance(e, ffi.SphError) else None, str(e)))]
        elif not candidates:
            state["lists"] = True   # (only the root keeps them)
        tm["host_decide_s"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        dist.broadcast_object_list(out, src=root)
        tm["gather_broadcast_s"] += time.perf_counter() - t0
        if out[0][0] is None:
            kind_, code, msg = out[0][1]
            if code is not None:
                raise ffi.SphError(code, f"adaptive step failed on rank {root}: {msg}")
            raise RuntimeError(f"adaptive step failed on rank {root} ({kind_}): {msg}")
        return out[0]

    def decide_compact(kind):
        """-> (ids, partner_c, counter_c) of the merged problem on every rank"""
        t0 = time.perf_counter()
        ctx.classify(p)
        counts = ctx.slab_partner_problem_prepare(kind, p, ap)
        mine = ctx.slab_partner_problem_download()
        tm["download_s"] += time.perf_counter() - t0
        parts = [None] * world if rank == root else None
        t0 = time.perf_counter()
        dist.gather_object(mine, parts, dst=root)
        tm["gather_broadcast_s"] += time.perf_counter() - t0
        out = [None]
        t0 = time.perf_counter()
        if rank == root:
            try:
                pids, *fields, off_c, idx_c = merge_slab_partner_problems(parts)
                out = [(pids,) + tuple(_decide_compact(ctx.lib, kind, pids, fields, off_c, idx_c, P, dt))]
            except Exception as e:  # noqa: BLE001 -- re-raised on every rank below
                out = [(None, (type(e).__name__, e.status if isinstance(e, ffi.SphError) else None, str(e)))]
        tm["host_decide_s"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        dist.broadcast_object_list(out, src=root)
        tm["gather_broadcast_s"] += time.perf_counter() - t0
        if out[0][0] is None:
            kind_, code, msg = out[0][1]
            if code is not None:
                raise ffi.SphError(code, f"adaptive step failed on rank {root}: {msg}")
            raise RuntimeError(f"adaptive step failed on rank {root} ({kind_}): {msg}")
        _count_slab_problem(count, kind, len(out[0][0]), [counts], 1)   # this rank's problem down, this rank's copy of the decisions up
        return out[0]

    def total(v):
        t = [None] * world
        dist.all_gather_object(t, v)
        return sum(t)

    n_before = total(ctx.n)
    info = {"n_before": n_before, "shares": 0, "merges": 0, "splits": 0}
    def mass_mine():
        count["bytes_down"] += 8 if candidates or compact else 4 * ctx.n
        return ctx.slab_sum_mass() if candidates or compact else float(ctx.download("mass").sum(dtype=np.float64))

    m1 = total(mass_mine())

    def apply(f, *a):
        t0 = time.perf_counter()
        f(*a)
        tm["apply_s"] += time.perf_counter() - t0

    if P.sharing:
        if compact:
            pids, mp, mc = decide_compact("share")
            info["shares"] = int(mc.sum())
            apply(ctx.slab_share_particles_compact, p, ap, pids, mp, mc)
        else:
            mp, mc = decide("share")
            info["shares"] = int(mc.sum())
            apply(ctx.share_particles, p, ap, mp, mc)
    if step_number % 2 == 0:
        if P.merging:
            if compact:
                pids, mp, mc = decide_compact("merge")
                info["merges"] = int(mc.sum())
                apply(ctx.slab_merge_particles_compact, p, ap, pids, mp, mc)
            else:
                mp, mc = decide("merge")
                info["merges"] = int(mc.sum())
                apply(ctx.merge_particles, p, ap, mp, mc)
    elif P.splitting:
        apply(ctx.classify, p)
        apply(ctx.split_particles, p, ap)
    info["n_after"] = total(ctx.n)
    info["seconds"] = tm
    info["splits"] = max(0, info["n_after"] - n_before) if step_number % 2 == 1 else 0
    m2 = total(mass_mine())
    if not abs(m1 - m2) <= 0.005:
        raise AssertionError(f"mass sum: {m1} vs {m2}")
    info["export"] = export
    info.update(count)
    return info


def compose_on_root(mine, compose, what: str, root: int = 0):
    """The tail of a per-process output flow (render.render_rank, sampling.sample_rank): every rank sends `root` its part through the
    launcher's process group (torch.distributed gather_object), `root` runs compose(parts).  Returns its result on `root`, None
    elsewhere; a failure on the root is re-raised on every rank as "<what> failed on rank <root>: ..."."""
    import torch.distributed as dist
    rank, world = dist.get_rank(), dist.get_world_size()
    parts = [None] * world if rank == root else None
    dist.gather_object(mine, parts, dst=root)
    out, result = [None], None
    if rank == root:
        try:
            result = compose(parts)
        except Exception as e:  # noqa: BLE001 -- re-raised on every rank below
            out = [(type(e).__name__, e.status if isinstance(e, ffi.SphError) else None, str(e))]
    dist.broadcast_object_list(out, src=root)
    if out[0] is not None:
        kind, code, msg = out[0]
        if code is not None:
            raise ffi.SphError(code, f"{what} failed on rank {root}: {msg}")
        raise RuntimeError(f"{what} failed on rank {root} ({kind}): {msg}")
    return result


def _launcher_total(v):
    """the sum of `v` over the ranks of the launcher's process group"""
    import torch.distributed as dist
    t = [None] * dist.get_world_size()
    dist.all_gather_object(t, v)
    return sum(t)


def rank_single_step_adaptivity_on_slabs_device(ctx: ffi.Context, P, dt: float, step_number: int, root: int = 0, relay_bytes: int = 0, total=None) -> dict:
    """single_step_adaptivity with ONE PROCESS PER RANK and the partner searches ON THE DEVICE (include/sph_rank_partner_search.h): per
    search every rank classifies, packs its local problem and relays it to `root` over the context's own transport, `root` merges,
    solves and validates on its device and relays the K decisions back, every rank applies its copy (Context.slab_find_partners_device,
    Context.slab_adapt_device: collective calls).  The same decisions and the same state as
    rank_single_step_adaptivity_on_slabs(export="compact"); no problem comes down, nothing is pickled, no decision goes up.  Every rank
    calls this after the same sph_step; a failure on the root inside merge or solve is raised on every rank.

    `relay_bytes`: the most bytes of one relay message (0: the transport's limit).  `total`: the sum of a number over all ranks, for
    the particle counts and the mass check (default: through the launcher's process group, torch.distributed; ranks that are threads
    of one process pass their own).

    info: the counts are this rank's, shaped like the group form's: ["passes"]: per search its kind, K ("participants"), this rank's
    local counts ("ranks": one triple), rounds, max_frontier, wide_rounds; ["bytes_down"]: the 48 B info struct per search and the 8 B
    device mass sums; ["bytes_up"]: 0; ["bytes_between_devices"]: what this rank sent and received in the relays; ["seconds"]: this
    rank's clock in the searches and the applies."""
    import time
    from .adaptivity import adapt_params
    if P.support_length_estimation != "FromMass":
        raise ValueError("rank_single_step_adaptivity_on_slabs_device: support_length_estimation must be FromMass")
    total = total or _launcher_total
    p, ap = P.to_ffi(), adapt_params(P, dt)
    info = {"n_before": total(ctx.n), "shares": 0, "merges": 0, "splits": 0, "export": "device", "exported_indices": 0, "bytes_down": 0, "bytes_up": 0,
            "bytes_between_devices": 0, "participants": 0, "passes": []}
    tm = {"find_s": 0.0, "apply_s": 0.0}

    def mass_sum():
        info["bytes_down"] += 8
        return total(ctx.slab_sum_mass())

    def search(kind):
        t0 = time.perf_counter()
        ctx.classify(p)
        found = ctx.slab_find_partners_device(kind, p, ap, root=root, relay_bytes=relay_bytes)
        moved = ctx.slab_relay_sizes()
        tm["find_s"] += time.perf_counter() - t0
        info["participants"] += found["participants"]
        info["exported_indices"] += found["local"][2]
        info["bytes_down"] += C_INFO_BYTES
        info["bytes_between_devices"] += moved["bytes_sent"] + moved["bytes_received"]
        info["passes"].append({"kind": kind, "participants": found["participants"], "ranks": [found["local"]], "rounds": found["rounds"],
                               "max_frontier": found["max_frontier"], "wide_rounds": found["wide_rounds"]})
        t0 = time.perf_counter()
        ctx.slab_adapt_device(kind, p, ap)
        tm["apply_s"] += time.perf_counter() - t0
        return found["transfers"]

    m1 = mass_sum()
    if P.sharing:
        info["shares"] = search("share")
    if step_number % 2 == 0:
        if P.merging:
            info["merges"] = search("merge")
    elif P.splitting:
        t0 = time.perf_counter()
        ctx.classify(p)
        ctx.split_particles(p, ap)
        tm["apply_s"] += time.perf_counter() - t0
    info["n_after"] = total(ctx.n)
    info["splits"] = max(0, info["n_after"] - info["n_before"]) if step_number % 2 == 1 else 0
    m2 = mass_sum()
    if not abs(m1 - m2) <= 0.005:
        raise AssertionError(f"mass sum: {m1} vs {m2}")
    info["seconds"] = tm
    return info


def rank_single_step_adaptivity(ctx: ffi.Context, gather: GatherContext, P, dt: float, step_number: int, capacity: int = 0, root: int = 0) -> dict:
    """The same adaptive step with ONE PROCESS PER RANK (the launch bench.py --gpus N and the RCCL / shared-memory transports use):
    every rank hands the fields adaptivity reads and its exported neighbour lists to `root` through the launcher's process group
    (torch.distributed gather_object: pickled numpy arrays -- host memory either way, the decisions are host code), `root`
    assembles them in global index order, runs the decisions and the device-side apply on its GatherContext (`gather`; None on
    the other ranks) and scatters every rank the particles of its slab, which it uploads with their new indices as ids.  Every
    rank calls this after the same sph_step; returns the step's counts (shares / merges / splits, n_after) on every rank."""
    import torch.distributed as dist
    if P.support_length_estimation != "FromMass":
        raise ValueError("rank_single_step_adaptivity: support_length_estimation must be FromMass")
    rank, world = dist.get_rank(), dist.get_world_size()
    mine = {f: ctx.download(f) for f in ("particle_id", "mass", "position", "velocity") + _ADAPT_FIELDS}
    mine["lists"] = ctx.download_neighbors()
    mine["cuts"] = ctx.dist_get_cuts()[:2]
    parts = [None] * world if rank == root else None
    dist.gather_object(mine, parts, dst=root)
    out = [None] * world
    if rank == root:
        # whatever goes wrong on the root between the gather and the scatter (the ids check, the 2^32-entries check, the mass-sum
        # assertion, an SphError of the gather context) must reach EVERY rank: the others sit in scatter_object_list meanwhile
        try:
            ids = [q["particle_id"] for q in parts]
            n = int(sum(len(i) for i in ids))
            allid = np.concatenate(ids)
            if not np.array_equal(np.sort(allid), np.arange(n, dtype=allid.dtype)):
                raise ValueError("rank_single_step_adaptivity: the particle ids of the ranks are not the indices 0 .. n-1")
            g = {}
            for f in ("mass", "position", "velocity") + _ADAPT_FIELDS:
                a = np.zeros((n,) + parts[0][f].shape[1:], parts[0][f].dtype)
                for q in parts:
                    a[q["particle_id"]] = q[f]
                g[f] = a
            new, info = _adapt_gathered(gather, P, dt, step_number, g, ids, [q["lists"] for q in parts], capacity)
            cuts = [-INF] + [float(q["cuts"][1]) for q in parts[:-1]] + [INF]
            for r, sel in enumerate(partition(new["position"][:, 0], cuts)):
                out[r] = ({f: new[f][sel] for f in new}, sel, info)
        except Exception as e:  # noqa: BLE001 -- re-raised on every rank below
            code = e.status if isinstance(e, ffi.SphError) else None
            out = [(None, None, (type(e).__name__, code, str(e)))] * world
    got = [None]
    dist.scatter_object_list(got, out if rank == root else None, src=root)
    if got[0][0] is None:
        kind, code, msg = got[0][2]
        if code is not None:
            raise ffi.SphError(code, f"adaptive step failed on rank {root}: {msg}")
        raise RuntimeError(f"adaptive step failed on rank {root} ({kind}): {msg}")
    new, sel, info = got[0]
    _reupload(ctx, {f: v for f, v in new.items()}, np.arange(len(sel)))
    ctx.upload_field("particle_id", sel.astype(np.uint32))
    return dict(info)


class ThreadedGroup:
    """k slab contexts of this process stepped the way the ranks of a multi-process run are: every rank calls sph_step on its OWN
    context from its OWN thread (a group of one member, rank-local branches and counts), the collectives meet in host memory
    (sph_thread_group_create / sph_comm_init_threads).  A collective that not every rank enters, ranks in different collectives or
    a send without a matching receive -- what would hang the RCCL transport -- comes back as an error."""

    def __init__(self, lib: ffi.SphLibrary, pos, mass, vel, planes, n_ranks: int, device_id: int = 0, capacities=None, cuts: Sequence[float] = None):
        import ctypes as C
        from concurrent.futures import ThreadPoolExecutor
        self.lib = lib
        self.group = C.c_void_p()
        rc = lib.thread_group_create(n_ranks, C.byref(self.group))
        if rc != 0:
            raise ffi.SphError(rc, "sph_thread_group_create failed")
        cuts = list(cuts) if cuts is not None else slab_cuts(pos[:, 0], n_ranks)   # (as make_loopback_group takes them)
        parts = partition(pos[:, 0], cuts)
        self.contexts = []
        for r in range(n_ranks):
            cap = capacities[r] if capacities is not None and capacities[r] else _slab_capacity(len(mass), n_ranks)
            c = ffi.Context(lib, cap, planes, device_id=device_id)
            c.dist_configure(r, n_ranks, cuts[r], cuts[r + 1])
            c.comm_init_threads(self.group, r, n_ranks)
            c.upload(mass[parts[r]], pos[parts[r]], vel[parts[r]])
            c.upload_field("particle_id", parts[r].astype(np.uint32))
            self.contexts.append(c)
        self.pool = ThreadPoolExecutor(n_ranks)

    def step(self, p):
        """One sph_step per rank, concurrently (ctypes drops the GIL inside the call).  Returns the ranks' stats; raises the first
        rank's error after ALL ranks have returned."""
        futs = [self.pool.submit(c.step, p) for c in self.contexts]
        out, err = [], None
        for f in futs:
            try:
                out.append(f.result())
            except ffi.SphError as e:
                err = err or e
        if err:
            raise err
        return out

    def close(self):
        self.pool.shutdown(wait=True)
        for c in self.contexts:
            c.close()
        self.contexts = []
        if self.group:
            self.lib.thread_group_destroy(self.group)
            self.group = None
