"""The adaptive half of configs[4]'s step with the full-list export against the candidate export (include/sph_candidates.h).

configs[4]'s scene and parameters exactly as bench.py's adaptivity leg builds them (adaptive_steps: ratio_stress_4m, EmptyAngle level
estimation, merging / sharing / splitting, the sizing radii of the two blocks), a few adaptive steps per mode from the same start, ONE
PROCESS PER MODE (fresh children of this script).  Writes <out-dir>/r8_candidates.json and a short r8_candidates.md: per mode the four
`seconds` buckets of AdaptivityDriver, the exported indices per step, the bytes that crossed the bus, the candidate kernels' profiler
times (from two further steps with the event profiler on: it perturbs dispatch, so those steps are not in the buckets) and the event
counts, which must be equal between the modes.  The comparison is candidates against lists in this run on this device.

    python scripts/gpu_candidates_time.py [--steps 4] [--warmup 2] [--out-dir profiles]
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
MODES = ("lists", "candidates")


def child(mode: str, steps: int, warmup: int) -> dict:
    import numpy as np
    import torch  # noqa: F401  (runtime load order, see ffi.load_product)
    from adaptive_sph_amd import ffi, scene as sc
    from adaptive_sph_amd.adaptivity import AdaptivityDriver, SplitPatterns
    from adaptive_sph_amd.workloads import WORKLOADS
    plib = ffi.load_product()
    scene_f, params_f, desc = WORKLOADS["ratio_stress_4m"]
    r_fine = float(np.sqrt(np.float32(0.0004385) ** 2 * 0.93 / np.pi))
    P = params_f(level_estimation_method="EmptyAngle", merging=True, sharing=True, splitting=True, particle_radius_fine=r_fine,
                 particle_radius_base=50 * r_fine, maximum_surface_distance=0.3)
    scn = scene_f()
    pos, mass, vel = sc.init_particles(scn)
    ctx = ffi.Context(plib, 2 * len(mass), sc.boundary_planes(scn.boundary, P.init_boundary_handler))
    ctx.upload(mass, pos, vel)
    drv = AdaptivityDriver(ctx, SplitPatterns.load_from_file(REPO / "tests" / "golden" / "split-patterns.yaml"), export=mode)
    p = P.to_ffi()
    for _ in range(warmup):
        ctx.step(p)
    if mode == "lists":
        ctx.download_neighbors(drv.host)   # (as bench.py: one untimed export, the device-side CSR buffers exist from here on)
    else:
        ctx.download_partner_candidates("merge", p, drv_ap(P), drv.host)
    per_step = []
    for _ in range(steps):
        t0 = time.perf_counter()
        st = ctx.step(p)
        t_step = time.perf_counter() - t0
        n = ctx.n
        info = drv.single_step_adaptivity(P, float(st.dt), int(st.step_number))
        passes = int(P.sharing) + int(P.merging and int(st.step_number) % 2 == 0)
        fields = passes * 21 * n                      # class (1) + mass, level, h2 (4 each) + position (8) per decision pass
        if mode == "lists":
            moved = fields + 4 * n + 4 * info["n_after"] + 4 * (n + 1) + 4 * info["exported_indices"]     # + the two mass vectors + the CSR
        else:
            moved = fields + passes * 4 * (n + 1) + 4 * info["exported_indices"] + 16                  # + a CSR per pass + two f64 sums
        per_step.append({"step_number": int(st.step_number), "n_before": n, "n_after": info["n_after"], "step_path_s": t_step,
                         "seconds": info["seconds"], "exported_indices": info["exported_indices"], "bytes_device_to_host": moved,
                         "events": {k: info[k] for k in ("shares", "merges", "splits")}})
    prof = {}
    ctx.profile_enable(1)
    ctx.profile_reset()
    prof_events = {"shares": 0, "merges": 0, "splits": 0}
    for _ in range(2):
        st = ctx.step(p)
        info = drv.single_step_adaptivity(P, float(st.dt), int(st.step_number))
        for k in prof_events:
            prof_events[k] += info[k]
    for name, (launches, ms) in ctx.profile_get().items():
        if name in ("candidates_count", "candidates_fill", "sum_mass", "classify"):
            prof[name] = {"scopes": launches, "total_ms": ms}
    ctx.profile_enable(0)
    out = {"mode": mode, "workload": desc, "particles": len(mass), "steps": steps, "warmup": warmup, "per_step": per_step,
           "profiled_steps": {"steps": 2, "events": prof_events, "scopes": prof}}
    ctx.close()
    return out


def drv_ap(P):
    from adaptive_sph_amd.adaptivity import adapt_params
    return adapt_params(P, 1e-3)


def mean(rows, f):
    return sum(f(r) for r in rows) / len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out-dir", default=str(REPO / "profiles"))
    ap.add_argument("--child", choices=MODES, default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds per mode")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.steps, a.warmup)), flush=True)
        return 0
    res = {}
    for mode in MODES:   # one process per mode; a mode that fails ends the run (nothing more is started on the device)
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", mode, "--steps", str(a.steps), "--warmup", str(a.warmup)],
                           capture_output=True, text=True, timeout=a.timeout)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return r.returncode or 1
        res[mode] = json.loads(line[-1][7:])
    ev = {m: [s["events"] for s in res[m]["per_step"]] for m in MODES}
    res["events_equal"] = ev["lists"] == ev["candidates"]
    out = Path(a.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    (out / "r8_candidates.json").write_text(json.dumps(res, indent=1) + "\n")
    L = ["# configs[4], adaptive half of the step: full-list export against candidate export", "",
         f"{res['lists']['particles']} particles, {a.steps} adaptive steps per mode after {a.warmup} plain steps, one process per mode, same start.",
         "Means per adaptive step; `seconds` buckets of `AdaptivityDriver` (host clock).", "",
         "| mode | download ms | host_decide ms | apply ms | mass_check ms | exported indices | MB device -> host |", "|---|---|---|---|---|---|---|"]
    for m in MODES:
        rows = res[m]["per_step"]
        b = {k: 1e3 * mean(rows, lambda r, k=k: r["seconds"][k]) for k in ("download", "host_decide", "apply", "mass_check")}
        L.append(f"| {m} | {b['download']:.2f} | {b['host_decide']:.2f} | {b['apply']:.2f} | {b['mass_check']:.2f} | "
                 f"{mean(rows, lambda r: r['exported_indices']):.0f} | {mean(rows, lambda r: r['bytes_device_to_host']) / 1e6:.1f} |")
    L += ["", "Per step (step number: events, exported indices):", ""]
    for m in MODES:
        L.append(f"- {m}: " + "; ".join(f"{s['step_number']}: {s['events']}, {s['exported_indices']}" for s in res[m]["per_step"]))
    L += ["", f"Event counts equal between the modes in every step: **{res['events_equal']}**.", "",
          "Profiler scopes over two further adaptive steps (event profiler on, not part of the buckets above):", ""]
    for m in MODES:
        L.append(f"- {m}: " + (", ".join(f"{k} {v['total_ms']:.3f} ms in {v['scopes']} scopes" for k, v in sorted(res[m]["profiled_steps"]["scopes"].items())) or "none"))
    (out / "r8_candidates.md").write_text("\n".join(L) + "\n")
    print("\n".join(L))
    return 0 if res["events_equal"] else 2


if __name__ == "__main__":
    sys.exit(main())
