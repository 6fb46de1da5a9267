"""Run under torch.distributed.run with N processes (tests/test_gpu_slab_sample_mp.py): every process is one rank of a slab
decomposition of a small dam break -- its own context, its own sph_step calls, the transport distributed.pick_transport chooses -- and
samples the group's fields through sampling.sample_rank: verdict words all-gathered and folded on every rank, (band, layer) gathered to
the root, composed on the root's context.  The root compares the raw planes with the numpy restatement (tests/sample_reference.py) fed
with the gathered fields; then one refusal that every rank must raise."""
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from adaptive_sph_amd import ffi, sampling, scene as sc  # noqa: E402
from adaptive_sph_amd.distributed import make_slab_context, pick_transport  # noqa: E402
from adaptive_sph_amd.workloads import default_params  # noqa: E402
from tests import sample_reference as sr  # noqa: E402

CH = ["density", "pressure", "velocity_x", "velocity_y", "level_estimation"]
FIELDS = ("particle_id", "mass", "position", "velocity", "density", "pressure", "level_estimation", "h2")


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
    ctx = make_slab_context(lib, pos, mass, vel, planes, rank, world, local, transport)
    for _ in range(4):
        ctx.step(p)
    mine = {f: ctx.download(f) for f in FIELDS}
    parts = [None] * world
    dist.all_gather_object(parts, mine)
    n = len(mass)
    f = {}
    for k in FIELDS[1:]:
        a = np.zeros((n,) + parts[0][k].shape[1:], parts[0][k].dtype)
        for q in parts:
            a[q["particle_id"]] = q[k]
        f[k] = a
    assert min(len(q["particle_id"]) for q in parts) > 0
    grid = sampling.GridSpec(91, 51, (-2.17, -1.18), 0.048)       # over the boundary box, three samples of overhang
    got = sampling.sample_rank(ctx, P, grid, CH, raw=True)
    # a refusal every rank must raise, with the same sentence: an explicit exponent that particles on both ranks reach
    tw = sr.Particles(f, CH, P.rest_density, P.maximum_surface_distance)
    vx = np.abs(f["velocity"][:, 0])
    e = sr.exponent_of(min(float(vx[q["particle_id"]].max()) for q in parts)) - 1
    exps = [None, None, e, None, None]
    idx, why = sr.first_offender(tw, exps)
    assert why == sr.BAD_CHANNEL + 2 and all((vx[q["particle_id"]] >= 2.0 ** e).any() for q in parts)
    try:
        sampling.sample_rank(ctx, P, grid, CH, exponents=exps)
        raise AssertionError("the exponent was not refused")
    except ffi.SphError as err:
        assert err.status == 1 and f"channel 2 (velocity) is not finite or not below 2^exponent = {2.0 ** e:g} (particle i={idx})" in str(err), str(err)
    if rank == 0:
        want, exps_auto, touching, (max_foot, pairs) = sr.sample(f, CH, P.rest_density, P.maximum_surface_distance, grid.nx, grid.ny, grid.origin, grid.spacing)
        raw = np.stack([got.raw[k] for k in ["weight"] + CH])
        assert np.array_equal(raw, want), [int(np.count_nonzero(raw[k] != want[k])) for k in range(len(raw))]
        assert want[0].any() and list(got.exponents.values()) == exps_auto
        assert (got.n_touching, got.max_footprint, got.n_pairs) == (touching, max_foot, pairs)
        values = np.stack([got.planes[k] for k in ["weight"] + CH])
        assert np.array_equal(values.view(np.uint32), sampling.resolve(raw, exps_auto).view(np.uint32))
        print(f"MP_SAMPLE OK world={world} transport={transport}", flush=True)
    else:
        assert got is None
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
