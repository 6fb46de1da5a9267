"""Run under torch.distributed.run with N processes (tests/test_gpu_slab_probe_mp.py): every process is one rank of a slab decomposition
of a small dam break -- its own context, its own sph_step calls, the transport distributed.pick_transport chooses -- and holds a
replica of two probe sets.  A gauge set is sampled through ProbeSet.sample_rank (verdict words all-gathered and folded on every rank,
compact layers gathered to the root, composed on the root's replica); the root compares the raw words with the numpy restatement
(tests/probe_reference.py) fed with the gathered fields.  Then 3 x (step, ProbeSet.advect_rank) on a tracer set: every rank's points
are all-gathered, identical, and equal to the twin's; then one refusal that every rank must raise."""
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from adaptive_sph_amd import ffi, probes, sampling, scene as sc  # noqa: E402
from adaptive_sph_amd.distributed import make_slab_context, pick_transport  # noqa: E402
from adaptive_sph_amd.workloads import default_params  # noqa: E402
from tests import probe_reference as pr  # noqa: E402
from tests import sample_reference as sr  # noqa: E402

CH = ["density", "pressure", "velocity_x", "velocity_y", "level_estimation"]
VEL = ["velocity_x", "velocity_y"]
FIELDS = ("particle_id", "mass", "position", "velocity", "density", "pressure", "level_estimation", "h2")


def gathered(ctx, n, world):
    """-> (the group's fields by global id, the ranks' ids)"""
    parts = [None] * world
    dist.all_gather_object(parts, {f: ctx.download(f) for f in FIELDS})
    f = {}
    for k in FIELDS[1:]:
        a = np.zeros((n,) + parts[0][k].shape[1:], parts[0][k].dtype)
        for q in parts:
            a[q["particle_id"]] = q[k]
        f[k] = a
    return f, [q["particle_id"] for q in parts]


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local)
    transport = pick_transport(world)
    dist.init_process_group("nccl" if transport == "rccl" else "gloo", rank=rank, world_size=world)
    lib = ffi.load_product()
    scn = sc.dam_break_small(40, 32, 1.0 / 40)
    pos, mass, vel = sc.init_particles(scn)
    P = default_params(merging=False, sharing=False, splitting=False, constrain_neighborhood_count=True, max_dt=0.004, maximum_surface_distance=0.2)
    planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    p = P.to_ffi()
    n = len(mass)
    ctx = make_slab_context(lib, pos, mass, vel, planes, rank, world, local, transport)
    for _ in range(4):
        ctx.step(p)
    f, ids = gathered(ctx, n, world)
    assert min(len(i) for i in ids) > 0
    x = f["position"][:, 0]
    cut = 0.5 * (float(x[ids[0]].max()) + float(x[ids[1]].min())) if x[ids[0]].max() < x[ids[1]].min() else float(np.median(x))
    ymid = float(np.median(f["position"][:, 1]))
    rng = np.random.default_rng(41)           # (the same seed on every rank: a replica)
    pts = np.concatenate([probes.line((cut - 0.2, ymid), (cut + 0.2, ymid), 64),
                          rng.uniform([-2.1, -1.1], [-0.7, 0.1], (200, 2)).astype(np.float32)])
    gauge = probes.ProbeSet(ctx, pts)
    got = gauge.sample_rank(P, CH, raw=True)
    if rank == 0:
        tw = pr.Particles(f, CH, P.rest_density, P.maximum_surface_distance)
        exps = pr.exponents(tw)
        want, foot, touched = pr.raw_at_points(tw, exps, pts[:, 0], pts[:, 1])
        raw = np.stack([got.raw[k] for k in ["weight"] + CH])
        assert np.array_equal(raw, want), [int(np.count_nonzero(raw[k] != want[k])) for k in range(len(raw))]
        assert want[0, :64].any() and list(got.exponents.values()) == exps
        assert (got.n_touching, got.n_pairs, got.n_touched_points) == (int((foot > 0).sum()), int(foot.sum()), int(touched.sum()))
        values = np.stack([got["weight"]] + [got[k] for k in CH])
        assert np.array_equal(values.view(np.uint32), sampling.resolve(raw[:, None, :], exps)[:, 0].view(np.uint32))
    else:
        assert got is None
    # tracers at every 3rd initial particle
    tracers = probes.ProbeSet(ctx, pos[::3])
    now = pos[::3].astype(np.float32)
    for step in range(3):
        dt = float(ctx.step(p).dt)
        info = tracers.advect_rank(P, dt)
        f, ids = gathered(ctx, n, world)
        tw = pr.Particles(f, VEL, P.rest_density, P.maximum_surface_distance, "rest")
        exps = pr.exponents(tw)
        raw, foot, _ = pr.raw_at_points(tw, exps, now[:, 0], now[:, 1])
        X, Y, moved = pr.advect(raw, exps, now[:, 0], now[:, 1], dt, 0.5)
        mine = tracers.points()
        everyone = [None] * world
        dist.all_gather_object(everyone, mine)
        want = np.stack([X, Y], axis=1)
        for r, theirs in enumerate(everyone):
            assert np.array_equal(theirs.view(np.uint32), want.view(np.uint32)), (step, r, int(np.count_nonzero(theirs != want)))
        assert (int(info.n_moved), int(info.n_stalled)) == (int(moved.sum()), int((~moved).sum())) and info.n_moved > 0
        assert [info.exponents[0], info.exponents[1]] == exps and int(info.n_pairs) == int(foot.sum())
        now = want
    # a refusal every rank must raise, with the same sentence: an explicit exponent that particles on both ranks reach
    tw = pr.Particles(f, CH, P.rest_density, P.maximum_surface_distance)
    vx = np.abs(f["velocity"][:, 0])
    e = sr.exponent_of(min(float(vx[i].max()) for i in ids)) - 1
    exps = [None, None, e, None, None]
    idx, why = pr.first_offender(tw, exps)
    assert why == sr.BAD_CHANNEL + 2 and all((vx[i] >= 2.0 ** e).any() for i in ids)
    try:
        gauge.sample_rank(P, CH, exponents=exps)
        raise AssertionError("the exponent was not refused")
    except ffi.SphError as err:
        assert err.status == 1 and f"channel 2 (velocity) is not finite or not below 2^exponent = {2.0 ** e:g} (particle i={idx})" in str(err), str(err)
    assert np.array_equal(tracers.points().view(np.uint32), now.view(np.uint32))
    if rank == 0:
        print(f"MP_PROBE OK world={world} transport={transport}", flush=True)
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
