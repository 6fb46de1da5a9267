"""Time of the device's field sampling (include/sph_sample.h) for configs[1] (1 M uniform particles) and configs[4] (4 M particles at
50:1 radii) on grids of 1024 x 512 and 2000 x 1000 samples over the scene's boundary box, with 1 channel (density) and 5 (density,
pressure, velocity x / y, level_estimation), against the first leg of the host alternative: downloading the fields a host sum reads.

Per case: the median wall clock of 10 calls of Context.sample_grid after 3 warm-ups (range pass, clear, scatter, resolve and the
download of the f32 planes: what the call costs its caller), then 10 calls under the library's event profiler for the mean time of
each kernel, and from the scatter's time the rate of its 64-bit integer atomics in bytes added per second (pairs x planes x 8 B).
usage: python scripts/gpu_sample_time.py [OUT.json [OUT.md]]"""
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from adaptive_sph_amd import ffi, sampling, scene as sc  # noqa: E402
from adaptive_sph_amd.workloads import WORKLOADS  # noqa: E402

CHANNELS = {1: ["density"], 5: ["density", "pressure", "velocity", "level"]}
HOST_FIELDS = {1: ["position", "mass", "h2", "density"], 5: ["position", "mass", "h2", "density", "pressure", "velocity", "level_estimation"]}
F32_ATOMIC_RATE = 1.3e12   # bytes added per second, global f32 atomic adds on this chip (the guide's figure)


def median_ms(f, reps=10, warm=3):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


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
        p = P.to_ffi()
        ctx.step(p)
        h = ctx.download("h2")
        rec = {"n": ctx.n, "h_min": float(h.min()), "h_max": float(h.max()), "cases": []}
        host = ffi.HostBuffers()   # persistent, touched host memory on both sides of the comparison
        for C in (1, 5):
            rec[f"host_download_{C}ch_ms"] = median_ms(lambda: [ctx.download(f, host) for f in HOST_FIELDS[C]])
        for nx, ny in ((1024, 512), (2000, 1000)):
            spacing = max(scn.boundary.width / nx, scn.boundary.height / ny)
            grid = sampling.GridSpec(nx, ny, (-0.5 * scn.boundary.width, -0.5 * scn.boundary.height), spacing)
            for C, channels in CHANNELS.items():
                sp = sampling.sample_params(grid, sampling.expand_channels(channels))
                _, _, info = ctx.sample_grid(p, sp, host=host)
                case = {"grid": [nx, ny], "spacing": spacing, "channels": C, "pairs": int(info.n_pairs), "touching": int(info.n_touching),
                        "max_footprint": int(info.max_footprint)}
                case["call_ms"] = median_ms(lambda: ctx.sample_grid(p, sp, host=host))
                case["call_fresh_arrays_ms"] = median_ms(lambda: ctx.sample_grid(p, sp))
                ctx.profile_enable(1)
                ctx.profile_reset()
                for _ in range(10):
                    ctx.sample_grid(p, sp, host=host)
                prof = ctx.profile_get()
                ctx.profile_enable(0)
                case["kernels_ms"] = {k: v[1] / max(v[0], 1) for k, v in prof.items() if k.startswith("sample")}
                scatter_s = case["kernels_ms"].get("sample_scatter", 0.0) * 1e-3
                case["atomic_bytes"] = case["pairs"] * (C + 1) * 8
                case["atomic_bytes_per_s"] = case["atomic_bytes"] / scatter_s if scatter_s > 0 else None
                rec["cases"].append(case)
                print(name, json.dumps(case), flush=True)
        ctx.close()
        out[name] = rec
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text(json.dumps(out, indent=1))
    if len(sys.argv) > 2:
        lines = ["| scene | grid | channels | pairs | call ms | call ms, fresh arrays | range ms | scatter ms | resolve ms | host download ms | atomic GB/s | of 1.3 TB/s |",
                 "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for name, rec in out.items():
            for c in rec["cases"]:
                k = c["kernels_ms"]
                rate = c["atomic_bytes_per_s"] or 0.0
                lines.append(f"| {name} ({rec['n']}) | {c['grid'][0]} x {c['grid'][1]} | {c['channels']} | {c['pairs']} | {c['call_ms']:.3f} | {c['call_fresh_arrays_ms']:.3f} | "
                             f"{k.get('sample_range', 0):.3f} | {k.get('sample_scatter', 0):.3f} | {k.get('sample_resolve', 0):.3f} | "
                             f"{rec['host_download_%dch_ms' % c['channels']]:.3f} | {rate / 1e9:.0f} | {rate / F32_ATOMIC_RATE:.2f} |")
        Path(sys.argv[2]).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
