"""Run under torch.distributed.run (tests/test_gpu_rank_partner_search_mp.py): the partner searches on the device with ONE PROCESS PER RANK
over the transport SPH_TRANSPORT names (shm: the shared-memory segment; ipc: the peer-mapped push transport, whose receiver reads its
inbox in place).  Every rank holds TWO slab contexts of the same launch with the same cuts: one takes the per-rank "compact" mode
(distributed.rank_single_step_adaptivity_on_slabs: local problems pickled to the root, numpy merge, host loop, decisions pickled back),
one the device mode (distributed.rank_single_step_adaptivity_on_slabs_device: relay, merge and solve on the root's device, relay).
Three adaptive steps; every rank compares the decisions of every pass and its final fields between the two, bit for bit.

MP_RANK_ROOT: the root.  MP_RANK_SCENE: "default" or "half" (the default scene at half spacing).  MP_RANK_BYTES_PER_SIDE: the transports'
message limit (0: the launcher's default); MP_RANK_EXPECT_CHUNKS=1: some blob must exceed it, so that the relay really cuts it."""
import os
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import yaml  # noqa: E402

from adaptive_sph_amd import adaptivity as A, distributed as D, ffi, scene as sc  # noqa: E402
from adaptive_sph_amd.workloads import default_params  # noqa: E402

RADII = dict(particle_radius_fine=0.012, particle_radius_base=0.05, maximum_surface_distance=0.3)   # tests/test_gpu_slab_candidates.py
FIELDS = ("mass", "position", "velocity", "h2", "h2_next", "level_estimation", "level_old", "particle_size_class")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    transport = D.pick_transport(world)
    dist.init_process_group("nccl" if transport == "rccl" else "gloo", rank=rank, world_size=world)
    root = int(os.environ.get("MP_RANK_ROOT", "0"))
    per_side = int(os.environ.get("MP_RANK_BYTES_PER_SIDE", "0")) or None
    expect_chunks = os.environ.get("MP_RANK_EXPECT_CHUNKS") == "1"
    lib = ffi.load_product()
    P = default_params(**RADII)
    doc = yaml.safe_load((REPO / "tests" / "golden" / "default-scene.yaml").read_text())
    scene_name = os.environ.get("MP_RANK_SCENE", "default")
    if scene_name == "half":
        for b in doc["blocks"]:
            b["spacing"] = b["spacing"] * 0.5
    scn = sc.SceneConfig.from_mapping(doc)
    sp = A.SplitPatterns.load_from_file(REPO / "tests" / "golden" / "split-patterns.yaml")
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    p = P.to_ffi()
    # the first set of inner cuts (MP_RANK_CUTS: "a,b;a,b;...") that the ranks accept: a slab narrower than two ghost layers is refused by
    # the first step, on every rank alike
    first = None
    for inner in os.environ["MP_RANK_CUTS"].split(";"):
        cuts = [-D.INF] + [float(v) for v in inner.split(",")] + [D.INF]
        assert len(cuts) == world + 1
        twins = {mode: D.make_slab_context(lib, pos, mass, vel, planes, rank, world, local, transport, cuts=cuts, bytes_per_side=per_side) for mode in ("compact", "device")}
        for c in twins.values():
            c.set_split_patterns(sp.patterns)
        try:
            first = {mode: c.step(p) for mode, c in twins.items()}
            break
        except ffi.SphError as e:
            if e.status != 30:
                raise
            for c in twins.values():
                c.close()
    assert first is not None, "the ranks accepted none of the cuts"
    decisions = {mode: [] for mode in twins}
    # what each mode applies, pass by pass: recorded in front of the apply calls
    a, b = twins["compact"], twins["device"]
    for name in ("slab_share_particles_compact", "slab_merge_particles_compact"):
        def compact_apply(p_, ap_, ids, mp, mc, inner=getattr(a, name), kind=name.split("_")[1]):
            decisions["compact"].append((kind, np.array(ids), np.array(mp), np.array(mc)))
            return inner(p_, ap_, ids, mp, mc)
        setattr(a, name, compact_apply)
    found, chunked = [], []
    inner_find, inner_adapt = b.slab_find_partners_device, b.slab_adapt_device

    def device_find(kind, *args, **kw):
        out = inner_find(kind, *args, **kw)
        found.append(out)
        sizes = b.slab_relay_sizes()
        chunked.append(max(sizes["bytes_of_rank"] + [sizes["decisions_bytes"]]) > sizes["chunk_bytes"])
        if per_side:
            assert sizes["chunk_bytes"] <= per_side, sizes
        if len(found) <= 2:
            print(f"MP_RANK_DEVICE rank={rank} search {len(found)} ({kind}): K={out['participants']} local={out['local']} {sizes}", flush=True)
        return out

    def device_adapt(op, *args):
        decisions["device"].append((op,) + b.slab_download_partner_decisions(found[-1]["participants"]))
        return inner_adapt(op, *args)

    b.slab_find_partners_device, b.slab_adapt_device = device_find, device_adapt
    events = {"shares": 0, "merges": 0, "splits": 0}
    between = 0
    for s in range(3):
        sta, stb = (first["compact"], first["device"]) if s == 0 else (a.step(p), b.step(p))
        assert float(sta.dt) == float(stb.dt)
        ia = D.rank_single_step_adaptivity_on_slabs(a, P, float(sta.dt), int(sta.step_number), root=root, export="compact")
        ib = D.rank_single_step_adaptivity_on_slabs_device(b, P, float(stb.dt), int(stb.step_number), root=root)
        for k in events:
            assert ia[k] == ib[k], (s, k, ia[k], ib[k])
            events[k] += ib[k]
        assert ia["n_after"] == ib["n_after"] and a.n == b.n
        assert ib["bytes_up"] == 0 and ib["bytes_down"] == 48 * len(ib["passes"]) + 16
        between += ib["bytes_between_devices"]
    assert len(decisions["compact"]) == len(decisions["device"]) == 4, (len(decisions["compact"]), len(decisions["device"]))
    for (k1, *d1), (k2, *d2) in zip(decisions["compact"], decisions["device"]):
        assert k1 == k2 and all(np.array_equal(x, y) for x, y in zip(d1, d2)), (k1, k2)
    ida, idb = a.download("particle_id"), b.download("particle_id")
    oa, ob = np.argsort(ida), np.argsort(idb)
    assert np.array_equal(ida[oa], idb[ob])
    for f in FIELDS:
        assert same_bits(a.download(f)[oa], b.download(f)[ob]), f
    a.step(p)
    b.step(p)
    mine = {"events": events, "chunked": any(chunked), "between": between}
    parts = [None] * world
    dist.all_gather_object(parts, mine)
    if rank == 0:
        assert all(q["events"] == events for q in parts)
        assert events["shares"] > 0 and events["merges"] > 0, events
        assert events["splits"] > 0 or scene_name == "half", events   # (at half spacing nobody grows large enough to split in three steps)
        assert sum(q["between"] for q in parts) > 0
        if expect_chunks:
            assert all(q["chunked"] for q in parts), parts
        print(f"MP_RANK_DEVICE OK world={world} transport={transport} root={root} chunked={int(any(q['chunked'] for q in parts))} events={events} "
              f"between={[q['between'] for q in parts]} cuts={cuts[1:-1]}", flush=True)
    dist.barrier()
    for c in twins.values():
        c.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except BaseException:   # noqa: BLE001
        import traceback
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(1)
