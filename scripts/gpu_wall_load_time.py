"""Time of the wall loads (include/sph_wall_load.h) on configs[1] (1 M uniform particles) after a few steps, against what the call
replaces on the same context in the same run: sph_download of mass, position, h2, density and pressure of every particle into persistent,
touched host buffers (the boundary would then have to be restated on the host; that time is not counted).

`reps` interleaved repeats of the three (wall load, wall load with a 64-bin profile along every plane, the download), the median wall
clock of each (every one ends in a device synchronise inside the library); then 20 calls under the library's event profiler for the mean
time of each pass, and from the 28 bytes a pass reads per particle (pm 16, id 4, density 4, pressure 4) its achieved bytes per second.
`--download-only` times the download alone (a build without wall loads).
usage: python scripts/gpu_wall_load_time.py [--download-only] [OUT.json [OUT.md]]"""
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from adaptive_sph_amd import ffi, scene as sc  # noqa: E402
from adaptive_sph_amd.workloads import WORKLOADS  # noqa: E402

HOST_FIELDS = ["mass", "position", "h2", "density", "pressure"]
PASS_BYTES = 28


def main(reps=15, steps=3):
    args = [a for a in sys.argv[1:] if a != "--download-only"]
    download_only = "--download-only" in sys.argv[1:]
    lib = ffi.load_product()
    name = "dam_break_1m"
    scene_f, params_f, _ = WORKLOADS[name]
    scn, P = scene_f(), params_f()
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    ctx = ffi.Context(lib, len(mass), planes)
    ctx.upload(mass, pos, vel)
    p = P.to_ffi()
    for _ in range(steps):
        ctx.step(p)
    host = ffi.HostBuffers()   # persistent, touched host memory: the download's best case

    def download():
        return {f: ctx.download(f, host) for f in HOST_FIELDS}

    cases = {"download": download}
    if not download_only:
        from adaptive_sph_amd import wall_loads
        ranges = wall_loads.plane_ranges(planes, scn.boundary)
        cases = {"wall_load": lambda: wall_loads.wall_load(ctx, p), "wall_load_64_bins": lambda: wall_loads.wall_load(ctx, p, 64, ranges), "download": download}
    for f in cases.values():   # warm up every shape
        for _ in range(3):
            f()
    ts = {k: [] for k in cases}
    for _ in range(reps):      # interleaved: the alternatives see the same machine
        for k, f in cases.items():
            t0 = time.perf_counter()
            f()
            ts[k].append(time.perf_counter() - t0)
    rec = {"n": ctx.n, "steps": steps, "reps": reps, "median_ms": {k: statistics.median(v) * 1e3 for k, v in ts.items()},
           "min_ms": {k: min(v) * 1e3 for k, v in ts.items()}, "max_ms": {k: max(v) * 1e3 for k, v in ts.items()},
           "download_bytes": int(sum(a.nbytes for a in download().values()))}
    if not download_only:
        load = wall_loads.wall_load(ctx, p)
        rec.update(n_entries=load.n_entries, n_wet=load.n_wet, normal=load.normal, force=load.force, peak=[load.peak_pressure(k) for k in range(load.n_elements)])
        ctx.profile_enable(1)
        ctx.profile_reset()
        for _ in range(20):
            wall_loads.wall_load(ctx, p)
        prof = ctx.profile_get()
        ctx.profile_enable(0)
        rec["kernels_ms"] = {k: v[1] / max(v[0], 1) for k, v in prof.items() if k.startswith("wall_load")}
        for k in ("wall_load_range", "wall_load_sums"):
            ms = rec["kernels_ms"].get(k)
            rec[k + "_bytes_per_s"] = ctx.n * PASS_BYTES / (ms * 1e-3) if ms else None
    print(name, json.dumps(rec), flush=True)
    ctx.close()
    if len(args) > 0:
        Path(args[0]).parent.mkdir(parents=True, exist_ok=True)
        Path(args[0]).write_text(json.dumps({name: rec}, indent=1))
    if len(args) > 1 and not download_only:
        m, k = rec["median_ms"], rec["kernels_ms"]
        lines = ["| scene | particles | wall load ms | with 64 bins per plane ms | download ms | range pass ms | sum pass ms | range GB/s | sums GB/s |",
                 "|---|---|---|---|---|---|---|---|---|",
                 f"| {name} | {rec['n']} | {m['wall_load']:.3f} | {m['wall_load_64_bins']:.3f} | {m['download']:.3f} | {k.get('wall_load_range', float('nan')):.4f} | "
                 f"{k.get('wall_load_sums', float('nan')):.4f} | {(rec['wall_load_range_bytes_per_s'] or 0) / 1e9:.0f} | {(rec['wall_load_sums_bytes_per_s'] or 0) / 1e9:.0f} |"]
        Path(args[1]).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
