"""Frame time of the device renderer (include/sph_render.h) at 2000 x 2000, S = 1 and 2, for configs[1] (1 M particles) and configs[4]
(4 M particles at 50:1 radii), against the host alternative's first leg: downloading position + mass + the visualised field.

Per case: the best of 5 wall-clock frames (colour pass + key clear + scatter + resolve + the 12 MB download, what Context.render_frame
costs the caller), then one frame under the library's event profiler for the per-kernel split.
usage: python scripts/gpu_render_time.py [OUT.json]"""
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from adaptive_sph_amd import ffi, render, scene as sc  # noqa: E402
from adaptive_sph_amd.workloads import WORKLOADS  # noqa: E402


def best_ms(f, reps=5):
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def main():
    out = {}
    lib = ffi.load_product()
    for name in ("dam_break_1m", "ratio_stress_4m"):
        scene_f, params_f, _ = WORKLOADS[name]
        scn, P = scene_f(), params_f()
        pos, mass, vel = sc.init_particles(scn)
        planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
        ctx = ffi.Context(lib, len(mass), planes)
        ctx.upload(mass, pos, vel)
        ctx.step(P.to_ffi())
        p = P.to_ffi()
        vis = render.VisualizationParams("Velocity")
        seg = render.boundary_segments(planes)
        rec = {"n": ctx.n}
        rec["host_download_position_mass_velocity_ms"] = best_ms(lambda: [ctx.download(f) for f in ("position", "mass", "velocity")])
        for S in (1, 2):
            rp = render.render_params(vis, P, 2000, 2000, S, 1.04, seg)
            ctx.render_frame(p, rp)   # buffers allocated on first use
            rec[f"S{S}_frame_ms"] = best_ms(lambda: ctx.render_frame(p, rp))
            ctx.profile_enable(1)
            ctx.profile_reset()
            ctx.render_frame(p, rp)
            prof = ctx.profile_get()
            ctx.profile_enable(0)
            rec[f"S{S}_kernels_ms"] = {k: v[1] for k, v in prof.items() if k.startswith("render")}
        ctx.close()
        out[name] = rec
        print(name, json.dumps(rec), flush=True)
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
