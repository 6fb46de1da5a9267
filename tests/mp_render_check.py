"""Run under torch.distributed.run with N processes (tests/test_gpu_slab_render_mp.py): every process is one rank of a slab
decomposition of a small dam break -- its own context, its own sph_step calls, the transport distributed.pick_transport chooses -- and
draws the group's frame through render.render_rank: pressure maximum all-gathered, (band, layer) gathered to the root, composed on the
root's context.  The root compares with the numpy restatement (tests/render_reference.py) fed with the gathered fields."""
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from adaptive_sph_amd import ffi, render, scene as sc  # noqa: E402
from adaptive_sph_amd.distributed import make_slab_context, pick_transport  # noqa: E402
from adaptive_sph_amd.workloads import default_params  # noqa: E402
from tests import render_reference as rr  # noqa: E402

FRAMES = [("Velocity", 300, 200, 1, 1.04), ("Pressure", 200, 200, 2, 1.0), ("RandomColor", 160, 250, 2, 0.9)]


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
    mine = {f: ctx.download(f) for f in ("particle_id", "mass", "position", "velocity", "pressure")}
    parts = [None] * world if rank == 0 else None
    dist.gather_object(mine, parts, dst=0)
    frames = [render.render_rank(ctx, P, render.VisualizationParams(attr), w, h, s, zoom, planes) for attr, w, h, s, zoom in FRAMES]
    try:
        render.render_rank(ctx, P, render.VisualizationParams("Velocity"), 64, 64, alpha=0.5)
        raise AssertionError("alpha was not refused")
    except ValueError:
        pass
    if rank == 0:
        n = len(mass)
        f = {}
        for k in ("mass", "position", "velocity", "pressure"):
            a = np.zeros((n,) + parts[0][k].shape[1:], parts[0][k].dtype)
            for q in parts:
                a[q["particle_id"]] = q[k]
            f[k] = a
        assert min(len(q["particle_id"]) for q in parts) > 0
        rad = rr.radii(f["mass"], P.rest_density)
        for (attr, w, h, s, zoom), got in zip(FRAMES, frames):
            cm = render.get_color_map(attr, P)
            stops = [] if cm is None else [(float(v), *map(float, c)) for v, c in cm.color_stops()]
            rgb = rr.colors(f, attr, 0, stops, P.rest_density, P.maximum_surface_distance)
            want = rr.Frame(w, h, s, zoom, render.boundary_segments(planes)).render(f["position"], rad, rgb)
            assert got is not None and got.shape == (h, w, 3)
            assert np.array_equal(got, want), (attr, int(np.sum(np.any(got != want, axis=2))))
            assert (got != 255).any()
        print(f"MP_RENDER OK world={world} transport={transport} frames={len(FRAMES)}", flush=True)
    else:
        assert all(fr is None for fr in frames)
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
