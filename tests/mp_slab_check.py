"""Run under torch.distributed.run with N processes (tests/test_gpu_multiprocess.py): every process is one rank of a slab
decomposition of a small dam break -- its own context, its own sph_step calls, the transport distributed.pick_transport chooses
(RCCL with one rank per GPU; the shared-memory transport when the ranks share a device) -- and rank 0 compares the gathered
result with a single context stepping the same scene.

Read before the rank's context is made (tests/test_gpu_multiprocess.py mixes the rank-local decisions of a row with them):
  MP_RANK_ENV   "r:NAME=VALUE;r:NAME=VALUE" -- environment of rank r only (the library reads its options at sph_create)
  MP_CUTS       "c1,c2,..": the world - 1 inner static cuts (default: equal particle counts)
  MP_FORMS      "1": every rank records per step which form its Jacobi exchanges took (fused push: ipc_pack_push in the profile) and
                which messages went through the multi-workgroup copy (ipc_copy); rank 0 prints them and checks MP_EXPECT_FORMS
  MP_EXPECT_FORMS  per rank, comma-separated: "F" fused in every step, "U" in none, "UF" a rank that starts empty: unfused for some
                steps, fused for the rest; "C" (any form) messages above SPH_IPC_COPY_MIN_BYTES went through the copy
  MP_REFUSE_AT  step s: rank 1 passes a max_iters one higher there -- every rank must be refused (status 1, "sph_params"), nothing
                poisoned; the run goes on with agreed parameters (and still ends bit for bit the loopback group's)
(SPH_HIP_LIBRARY selects the library, ffi.PRODUCT_LIB.)"""
import os
import re
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from adaptive_sph_amd import ffi, scene as sc  # noqa: E402
from adaptive_sph_amd.distributed import INF, make_slab_context, pick_transport  # noqa: E402
from adaptive_sph_amd.workloads import dam_break_params  # noqa: E402


def rank_env(rank):
    out = {}
    for item in filter(None, os.environ.get("MP_RANK_ENV", "").split(";")):
        r, kv = item.split(":", 1)
        name, val = kv.split("=", 1)
        if int(r) == rank:
            out[name] = val
    return out


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    os.environ.update(rank_env(rank))
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    transport = pick_transport(world)
    dist.init_process_group("nccl" if transport == "rccl" else "gloo", rank=rank, world_size=world)
    lib = ffi.load_product()
    scn = sc.dam_break_small(128, 64, 1 / 64)
    pos, mass, vel = sc.init_particles(scn)
    vel = vel.copy()
    vel[:, 0] = 0.8                                  # particles cross the cuts
    planes = sc.boundary_planes(scn.boundary)
    p = dam_break_params().to_ffi()
    steps = int(os.environ.get("MP_STEPS", "12"))
    cuts = None
    if os.environ.get("MP_CUTS"):
        cuts = [-INF] + [float(x) for x in os.environ["MP_CUTS"].split(",")] + [INF]
        assert len(cuts) == world + 1
    forms_on = os.environ.get("MP_FORMS") == "1"
    refuse_at = int(os.environ.get("MP_REFUSE_AT", "-1"))
    ctx = make_slab_context(lib, pos, mass, vel, planes, rank, world, local, transport, cuts=cuts)
    n_start = ctx.n
    if forms_on:
        ctx.profile_enable(1)
    its, forms, refusals = [], [], []
    for s in range(steps):
        if s == refuse_at:
            q = p
            if rank == 1:
                q = type(p).from_buffer_copy(p)
                q.max_iters = p.max_iters + 1
            try:
                ctx.step(q)
                refusals.append(None)
            except ffi.SphError as e:
                refusals.append((e.status, str(e)))
        if forms_on:
            ctx.profile_reset()
        st = ctx.step(p)
        its.append((float(st.dt), int(st.div_solver.iters), int(st.density_solver.iters)))
        if forms_on:
            prof = ctx.profile_get()
            forms.append(("ipc_pack_push" in prof, prof.get("ipc_copy", (0, 0.0))[0], ctx.dist_get_stats()["bytes_sent"]))
    mine = {f: ctx.download(f) for f in ("particle_id", "position", "velocity", "density", "neighbor_count")}
    stats = ctx.dist_get_stats()
    parts = [None] * world
    dist.all_gather_object(parts, (mine, its, stats, n_start, forms, refusals))
    if rank == 0:
        single = ffi.Context(lib, len(mass), planes, device_id=local)
        single.upload(mass, pos, vel)
        ref_its = []
        for _ in range(steps):
            st = single.step(p)
            ref_its.append((float(st.dt), int(st.div_solver.iters), int(st.density_solver.iters)))
        n = len(mass)
        ids = np.concatenate([q[0]["particle_id"] for q in parts])
        assert np.array_equal(np.sort(ids), np.arange(n)), "particles lost or duplicated"
        for q in parts:
            assert q[1] == parts[0][1], "ranks disagree on dt / iteration counts"
        # MP_SOAK (scripts/mp_ipc_soak.sh: hundreds of free-running steps): slabs and single context are two correct evaluations of a chaotic
        # scene and part ways after ~75 steps -- the soak keeps the exact checks (nothing lost, the ranks agree, BIT FOR BIT the loopback group)
        soak = bool(os.environ.get("MP_SOAK"))
        assert soak or all(abs(a[0] - b[0]) <= 1e-5 * b[0] and abs(a[1] - b[1]) <= 1 and abs(a[2] - b[2]) <= 1 for a, b in zip(parts[0][1], ref_its)), (parts[0][1][:20], ref_its[:20])
        for f, tol in (() if soak else (("position", 1e-5), ("velocity", 1e-3), ("density", 1e-4))):
            got = np.zeros_like(single.download(f))
            for q in parts:
                got[q[0]["particle_id"]] = q[0][f]
            ref = single.download(f)
            err = np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max()
            assert err <= tol, (f, err)
        cnt = np.zeros(n, np.uint32)
        for q in parts:
            cnt[q[0]["particle_id"]] = q[0]["neighbor_count"]
        assert soak or (cnt != single.download("neighbor_count")).mean() < 1e-3
        assert all(q[2]["exchanges"] > 0 and q[2]["bytes_sent"] > 0 for q in parts), [q[2] for q in parts]
        assert min(len(q[0]["particle_id"]) for q in parts) > 0 and len({len(q[0]["particle_id"]) for q in parts}) > 1     # particles migrated
        if refuse_at >= 0:
            for r, q in enumerate(parts):
                assert len(q[5]) == 1 and q[5][0] is not None and q[5][0][0] == 1 and "sph_params" in q[5][0][1], (r, q[5])
            print(f"MP_REFUSED every rank: {parts[0][5][0][1]}", flush=True)
        if forms_on:
            expect = os.environ.get("MP_EXPECT_FORMS", "").split(",") if os.environ.get("MP_EXPECT_FORMS") else []
            for r, q in enumerate(parts):
                seen = "".join("F" if f[0] else "U" for f in q[4])
                copies = sum(f[1] for f in q[4])
                sent = [f[2] for f in q[4]]
                big = max(b - a for a, b in zip([0] + sent, sent))
                print(f"MP_FORMS rank={r} start={q[3]} end={len(q[0]['particle_id'])} steps={seen} ipc_copy={copies} max_bytes_sent_per_step={big}", flush=True)
                want = expect[r] if r < len(expect) else ""
                if want in ("F", "U"):
                    assert seen == want * len(seen), (r, seen)
                elif want == "UF":   # unfused while it owned nothing and had no ghosts, fused from the step the column came into its reach
                    assert q[3] == 0 and re.fullmatch("U+F+", seen), (r, seen)
                elif want == "C":
                    thr = int(os.environ["SPH_IPC_COPY_MIN_BYTES"])
                    assert copies > 0 and big > thr, (r, copies, big, thr)
        # ... and BIT FOR BIT the loopback group's result (the same slabs as contexts of one process: the verification form of the
        # decomposition) -- whatever carried the messages, the ranks did the same arithmetic on the same particles in the same order
        from adaptive_sph_amd.distributed import make_loopback_group
        grp = make_loopback_group(lib, pos, mass, vel, planes, world, device_id=local, cuts=cuts)
        for _ in range(steps):
            ffi.group_step(grp, p)
        for r, (q, c) in enumerate(zip(parts, grp)):
            for f in ("particle_id", "position", "velocity", "density", "neighbor_count"):
                assert np.array_equal(q[0][f], c.download(f)), (r, f)
        for c in grp:
            c.close()
        print(f"MP_CHECK OK world={world} transport={transport} steps={steps}", flush=True)
    dist.barrier()
    ctx.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except BaseException:   # noqa: BLE001  (a rank that dies while the others sit in a collective would hang the launch)
        import traceback
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(1)
