"""Time of the state ledger (include/sph_ledger.h) with all groups on configs[1] (1 M uniform particles) and configs[4] (4 M particles at
50:1 radii) after a few steps, against what the call replaces on the same context in the same run: sph_download of position, velocity,
mass, density, pressure and h2 into persistent, touched host buffers, followed by the numpy reductions scripts/gpu_config3_divergence.py
prints (vmax, ymin, below the floor, rho_max) -- and against that download followed by ALL the ledger's quantities in numpy.

Per scene: `reps` interleaved repeats of the three (ledger, download + four reductions, download + everything), the median wall clock
of each (every one ends in a device synchronise inside the library); then 20 ledger calls under the library's event profiler for the
mean time of each pass, and from the bytes a pass reads (range: pm 16 + velocity 8 + id 4 + density 4 + pressure 4 = 36 B per particle;
sums: pm 16 + velocity 8 + density 4 = 28 B) its achieved bytes per second.
usage: python scripts/gpu_ledger_time.py [OUT.json [OUT.md]]"""
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from adaptive_sph_amd import ffi, ledger, scene as sc  # noqa: E402
from adaptive_sph_amd.workloads import WORKLOADS  # noqa: E402

HOST_FIELDS = ["position", "velocity", "mass", "density", "pressure", "h2"]
RANGE_BYTES, SUMS_BYTES = 36, 28


def divergence_reductions(f):
    """What scripts/gpu_config3_divergence.py prints after a step."""
    v = f["velocity"].astype(np.float64)
    x = f["position"]
    return (float(np.sqrt((v ** 2).sum(axis=1)).max()), float(x[:, 1].min()), int((x[:, 1] < -1.0).sum()), float(f["density"].max()))


def all_reductions(f, rest_density):
    """Everything the ledger returns, the plain numpy way (f64 sums, argmax / argmin for the ids)."""
    m, v, x = f["mass"].astype(np.float64), f["velocity"].astype(np.float64), f["position"].astype(np.float64)
    rho = f["density"].astype(np.float64)
    s2 = (f["velocity"] ** 2).sum(axis=1)
    out = [m.sum(), (m * v[:, 0]).sum(), (m * v[:, 1]).sum(), (m * x[:, 0]).sum(), (m * x[:, 1]).sum(), 0.5 * (m * (v ** 2).sum(axis=1)).sum(),
           (m * (x[:, 0] * v[:, 1] - x[:, 1] * v[:, 0])).sum(), (m / rho).sum(), np.maximum(rho - rest_density, 0.0).sum(), int(np.argmax(s2))]
    for a in (f["position"][:, 0], f["position"][:, 1], f["mass"], f["density"], f["pressure"], f["h2"]):
        out += [int(np.argmin(a)), int(np.argmax(a))]
    out.append(int(((np.abs(f["position"][:, 0]) > 2.0) | (np.abs(f["position"][:, 1]) > 1.0)).sum()))
    out.append(bool(all(np.isfinite(a).all() for a in f.values())))
    return out


def main(reps=15, steps=3):
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
        for _ in range(steps):
            ctx.step(p)
        host = ffi.HostBuffers()   # persistent, touched host memory: the download's best case

        def download():
            return {f: ctx.download(f, host) for f in HOST_FIELDS}

        cases = {"ledger": lambda: ledger.ledger(ctx, p),
                 "download": download,
                 "download_and_divergence_reductions": lambda: divergence_reductions(download()),
                 "download_and_all_reductions": lambda: all_reductions(download(), P.rest_density)}
        for f in cases.values():   # warm up every shape
            for _ in range(3):
                f()
        ts = {k: [] for k in cases}
        for _ in range(reps):      # interleaved: the alternatives see the same machine
            for k, f in cases.items():
                t0 = time.perf_counter()
                f()
                ts[k].append(time.perf_counter() - t0)
        led = ledger.ledger(ctx, p)
        vmax, ymin, below, rho_max = divergence_reductions(download())
        assert led.extreme("min_y")[0] == ymin and led.extreme("max_density")[0] == rho_max and abs(led.vmax - vmax) <= 1e-6 * vmax
        rec = {"n": ctx.n, "steps": steps, "reps": reps, "median_ms": {k: statistics.median(v) * 1e3 for k, v in ts.items()},
               "min_ms": {k: min(v) * 1e3 for k, v in ts.items()}, "max_ms": {k: max(v) * 1e3 for k, v in ts.items()},
               "vmax": led.vmax, "vmax_id": led.extreme("max_speed2")[1], "y_min": ymin, "rho_max": rho_max, "n_outside": led.n_outside,
               "download_bytes": int(sum(a.nbytes for a in download().values()))}
        ctx.profile_enable(1)
        ctx.profile_reset()
        for _ in range(20):
            ledger.ledger(ctx, p)
        prof = ctx.profile_get()
        ctx.profile_enable(0)
        rec["kernels_ms"] = {k: v[1] / max(v[0], 1) for k, v in prof.items() if k.startswith("ledger")}
        for k, b in (("ledger_range", RANGE_BYTES), ("ledger_sums", SUMS_BYTES)):
            ms = rec["kernels_ms"].get(k)
            rec[k + "_bytes_per_s"] = ctx.n * b / (ms * 1e-3) if ms else None
        print(name, json.dumps(rec), flush=True)
        ctx.close()
        out[name] = rec
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text(json.dumps(out, indent=1))
    if len(sys.argv) > 2:
        lines = ["| scene | particles | ledger ms | download ms | download + 4 reductions ms | download + all reductions ms | range pass ms | sum pass ms | range GB/s | sums GB/s |",
                 "|---|---|---|---|---|---|---|---|---|---|"]
        for name, r in out.items():
            m, k = r["median_ms"], r["kernels_ms"]
            lines.append(f"| {name} | {r['n']} | {m['ledger']:.3f} | {m['download']:.3f} | {m['download_and_divergence_reductions']:.3f} | "
                         f"{m['download_and_all_reductions']:.3f} | {k.get('ledger_range', float('nan')):.4f} | {k.get('ledger_sums', float('nan')):.4f} | "
                         f"{(r['ledger_range_bytes_per_s'] or 0) / 1e9:.0f} | {(r['ledger_sums_bytes_per_s'] or 0) / 1e9:.0f} |")
        Path(sys.argv[2]).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
