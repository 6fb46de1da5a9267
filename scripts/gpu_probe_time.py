"""Time of the device's probe sets (include/sph_probe.h) on dam_break_1m (1 M uniform particles) after the benchmark's warm-up of 20 steps:

  (a) 64 gauges on one vertical line (pressure, density, velocity): ProbeSet.sample
  (b) one tracer per particle: ProbeSet.sample of the velocity, then ProbeSet.advect

each beside two things measured in the same run: sph_sample_grid over a lattice with the same number of samples (a: 1 x 64 on the
line) or at the particle spacing over the boundary box (b) -- existing code with the same per-pair arithmetic -- and the download of
position, mass, h, density and velocity a host-side evaluation would need.  Medians of 10 calls after 3 warm-ups with the spread
(min .. max), then 10 calls under the library's event profiler for the mean time of each kernel; k_sample_range's time is the yardstick
of a bare streaming read of the particles.
usage: python scripts/gpu_probe_time.py [OUT.json [OUT.md]]"""
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from adaptive_sph_amd import ffi, probes, sampling, scene as sc  # noqa: E402
from adaptive_sph_amd.workloads import WORKLOADS  # noqa: E402

HOST_FIELDS = ["position", "mass", "h2", "density", "velocity"]
GAUGE_FIELDS = ["pressure", "density", "velocity"]
WARMUP_STEPS = 20


def timed(f, reps=10, warm=3):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def kernels(ctx, f, prefix, reps=10):
    ctx.profile_enable(1)
    ctx.profile_reset()
    for _ in range(reps):
        f()
    prof = ctx.profile_get()
    ctx.profile_enable(0)
    return {k: v[1] / max(v[0], 1) for k, v in prof.items() if k.startswith(prefix)}


def main():
    lib = ffi.load_product()
    scene_f, params_f, _ = WORKLOADS["dam_break_1m"]
    scn, P = scene_f(), params_f()
    pos, mass, vel = sc.init_particles(scn)
    ctx = ffi.Context(lib, len(mass), sc.boundary_planes(scn.boundary, P.init_boundary_handler))
    ctx.upload(mass, pos, vel)
    p = P.to_ffi()
    for _ in range(WARMUP_STEPS):
        ctx.step(p)
    host = ffi.HostBuffers()
    x = ctx.download("position")
    h = ctx.download("h2")
    out = {"n": ctx.n, "h": float(h.max()), "host_download": timed(lambda: [ctx.download(f, host) for f in HOST_FIELDS])}
    print("host_download", json.dumps(out["host_download"]), flush=True)

    # (a) 64 gauges on a vertical line through the middle of the fluid, from the floor to above the surface
    xm = float(np.median(x[:, 0]))
    y0, y1 = float(x[:, 1].min()), float(x[:, 1].max())
    line = probes.line((xm, y0), (xm, y1 + 0.1 * (y1 - y0)), 64)
    spacing = float(line[1, 1] - line[0, 1])
    lattice = sampling.GridSpec(1, 64, (xm - 0.5 * spacing, y0 - 0.5 * spacing), spacing)
    a = {"points": 64}
    with probes.ProbeSet(ctx, line) as g:
        v = g.sample(p, GAUGE_FIELDS)
        a.update(pairs=v.n_pairs, touching=v.n_touching, cells=[g.info.cells_x, g.info.cells_y], cell_size=g.info.cell_size)
        a["probe_sample"] = timed(lambda: g.sample(p, GAUGE_FIELDS))
        a["probe_kernels_ms"] = kernels(ctx, lambda: g.sample(p, GAUGE_FIELDS), ("probe", "sample"))
    a["lattice"] = timed(lambda: sampling.sample_grid(ctx, p, lattice, GAUGE_FIELDS, host=host))
    a["lattice_kernels_ms"] = kernels(ctx, lambda: sampling.sample_grid(ctx, p, lattice, GAUGE_FIELDS, host=host), "sample")
    out["gauges"] = a
    print("gauges", json.dumps(a), flush=True)

    # (b) one tracer per particle
    dx = min(float(blk.spacing) for blk in scn.blocks)
    grid = sampling.GridSpec.covering(scn.boundary, dx)
    b = {"points": ctx.n, "lattice_samples": grid.nx * grid.ny}
    with probes.ProbeSet(ctx, x) as t:
        v = t.sample(p, ["velocity"], volume="rest")
        b.update(pairs=v.n_pairs, touching=v.n_touching, cells=[t.info.cells_x, t.info.cells_y], cell_size=t.info.cell_size)
        b["probe_sample"] = timed(lambda: t.sample(p, ["velocity"], volume="rest"))
        b["probe_kernels_ms"] = kernels(ctx, lambda: t.sample(p, ["velocity"], volume="rest"), ("probe", "sample"))
        b["probe_advect"] = timed(lambda: t.advect(p, 1e-4))   # (sample, move, and the next call bins again)
        b["advect_kernels_ms"] = kernels(ctx, lambda: t.advect(p, 1e-4), ("probe", "sample"))
    lat = sampling.sample_grid(ctx, p, grid, ["velocity"], volume="rest", host=host)
    b["lattice_pairs"] = lat.n_pairs
    b["lattice"] = timed(lambda: sampling.sample_grid(ctx, p, grid, ["velocity"], volume="rest", host=host))
    b["lattice_kernels_ms"] = kernels(ctx, lambda: sampling.sample_grid(ctx, p, grid, ["velocity"], volume="rest", host=host), "sample")
    out["tracers"] = b
    print("tracers", json.dumps(b), flush=True)
    ctx.close()

    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text(json.dumps(out, indent=1))
    if len(sys.argv) > 2:
        def cell(t):
            return f"{t['median_ms']:.3f} ({t['min_ms']:.3f} .. {t['max_ms']:.3f})"
        lines = [f"dam_break_1m, {out['n']} particles, after {WARMUP_STEPS} steps; median ms of 10 calls after 3 warm-ups (min .. max)", "",
                 "| case | points | pairs | probe call | lattice call (samples) | host download |", "|---|---|---|---|---|---|",
                 f"| (a) gauges: sample | 64 | {a['pairs']} | {cell(a['probe_sample'])} | {cell(a['lattice'])} (64) | {cell(out['host_download'])} |",
                 f"| (b) tracers: sample | {b['points']} | {b['pairs']} | {cell(b['probe_sample'])} | {cell(b['lattice'])} ({b['lattice_samples']}) | {cell(out['host_download'])} |",
                 f"| (b) tracers: advect | {b['points']} | {b['pairs']} | {cell(b['probe_advect'])} | | |", "",
                 "mean kernel ms under the event profiler:", ""]
        for name, k in (("(a) probe", a["probe_kernels_ms"]), ("(a) lattice", a["lattice_kernels_ms"]), ("(b) probe sample", b["probe_kernels_ms"]),
                        ("(b) probe advect", b["advect_kernels_ms"]), ("(b) lattice", b["lattice_kernels_ms"])):
            lines.append(f"- {name}: " + ", ".join(f"{n} {ms:.3f}" for n, ms in sorted(k.items())))
        Path(sys.argv[2]).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
