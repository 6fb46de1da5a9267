"""The adaptive half of configs[4]'s step with the full-list export, the candidate export (include/sph_candidates.h), the compact
partner problem (include/sph_partner_problem.h) and the search on the device (include/sph_partner_search.h).

configs[4]'s scene and parameters exactly as bench.py's adaptivity leg builds them (adaptive_steps: ratio_stress_4m, EmptyAngle level
estimation, merging / sharing / splitting, the sizing radii of the two blocks), a few adaptive steps per mode from the same start, ONE
PROCESS PER MODE AND REPEAT (fresh children of this script).  Writes <out-dir>/<name>.json and a short <name>.md: per mode the four
`seconds` buckets of AdaptivityDriver, per partner search (pass) its participants, exported indices, bytes down / up and its share of
the buckets, the kernels' profiler times (from two further steps with the event profiler on: it perturbs dispatch, so those steps are
not in the buckets) and the event counts, which must be equal between the modes.  The comparison is between the modes in this run on
this device; --repeats gives the run-to-run spread.

--config 0 runs BASELINE configs[0] instead (the default config on the default scene, 1 035 particles).  In device mode every pass also
reports its search (K, rounds, max_frontier, wide_rounds); --wide-threshold and SPH_SEARCH_BLOCK (laboratory build, SPH_HIP_LIBRARY)
select the alternatives to the library's defaults.

    python scripts/gpu_candidates_time.py [--steps 2] [--warmup 2] [--repeats 2] [--out-dir profiles] [--name r9_compact_problem]
                                          [--modes lists,candidates,compact,device] [--config 4]
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
MODES = ("lists", "candidates", "compact", "device")


def child(mode: str, steps: int, warmup: int, config: int = 4, wide_threshold: int = 0) -> dict:
    import numpy as np
    import torch  # noqa: F401  (runtime load order, see ffi.load_product)
    from adaptive_sph_amd import ffi, scene as sc
    from adaptive_sph_amd.adaptivity import AdaptivityDriver, SplitPatterns
    from adaptive_sph_amd.workloads import WORKLOADS
    plib = ffi.load_product()
    if config == 0:
        from adaptive_sph_amd.workloads import default_params
        P, desc = default_params(), "configs[0]: the default config on the default scene"
        scn = sc.SceneConfig.from_yaml(str(REPO / "tests" / "golden" / "default-scene.yaml"))
    else:
        scene_f, params_f, desc = WORKLOADS["ratio_stress_4m"]
        r_fine = float(np.sqrt(np.float32(0.0004385) ** 2 * 0.93 / np.pi))
        P = params_f(level_estimation_method="EmptyAngle", merging=True, sharing=True, splitting=True, particle_radius_fine=r_fine,
                     particle_radius_base=50 * r_fine, maximum_surface_distance=0.3)
        scn = scene_f()
    pos, mass, vel = sc.init_particles(scn)
    ctx = ffi.Context(plib, max(2 * len(mass), 120000), sc.boundary_planes(scn.boundary, P.init_boundary_handler))
    ctx.upload(mass, pos, vel)
    drv = AdaptivityDriver(ctx, SplitPatterns.load_from_file(REPO / "tests" / "golden" / "split-patterns.yaml"), export=mode)
    p = P.to_ffi()
    if mode == "device" and wide_threshold:
        inner = ctx.find_partners_device
        ctx.find_partners_device = lambda kind, pp, ap, thr=0: inner(kind, pp, ap, wide_threshold)
    for _ in range(warmup):
        ctx.step(p)
    if mode == "lists":
        ctx.download_neighbors(drv.host)   # (as bench.py: one untimed export, the device-side CSR buffers exist from here on)
    elif mode == "candidates":
        ctx.download_partner_candidates("merge", p, drv_ap(P), drv.host)
    elif mode == "compact":
        ctx.download_partner_problem("merge", p, drv_ap(P), drv.host)
    else:
        ctx.classify(p)
        ctx.find_partners_device("merge", p, drv_ap(P))   # (untimed: the search's buffers exist from here on)
    per_step = []
    for _ in range(steps):
        t0 = time.perf_counter()
        st = ctx.step(p)
        t_step = time.perf_counter() - t0
        n = ctx.n
        info = drv.single_step_adaptivity(P, float(st.dt), int(st.step_number))
        moved = info["bytes_down"]   # (the driver counts what its exports moved: adaptivity.AdaptivityDriver)
        per_step.append({"step_number": int(st.step_number), "n_before": n, "n_after": info["n_after"], "step_path_s": t_step,
                         "seconds": info["seconds"], "exported_indices": info["exported_indices"], "bytes_device_to_host": moved,
                         "bytes_host_to_device": info["bytes_up"], "participants": info["participants"], "passes": info["passes"],
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
        if name in ("candidates_count", "candidates_fill", "problem_mark", "problem_pack", "problem_expand", "search_writers", "search_rounds", "search_validate",
                    "sum_mass", "classify"):
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
    ap.add_argument("--steps", type=int, default=2, help="adaptive steps per mode (2: one odd step with a split, one even step with a merge)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=2, help="processes per mode: the spread between them is the run-to-run spread")
    ap.add_argument("--out-dir", default=str(REPO / "profiles"))
    ap.add_argument("--name", default="r9_compact_problem")
    ap.add_argument("--child", choices=MODES, default=None)
    ap.add_argument("--modes", default=",".join(MODES), help="comma-separated subset of " + ",".join(MODES) + " (lists is the reference of the event counts)")
    ap.add_argument("--config", type=int, choices=(0, 4), default=4, help="BASELINE configs[4] (ratio_stress_4m) or configs[0] (the default config and scene)")
    ap.add_argument("--wide-threshold", type=int, default=0, help="device mode: sph_find_partners_device's wide_threshold (0: the library's default)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per process")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.steps, a.warmup, a.config, a.wide_threshold)), flush=True)
        return 0
    modes = tuple(m for m in MODES if m in a.modes.split(","))
    res = {m: [] for m in modes}
    for rep in range(a.repeats):
        for mode in modes:   # one process per mode and repeat; a process that fails ends the run (nothing more is started on the device)
            r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", mode, "--steps", str(a.steps), "--warmup", str(a.warmup),
                                "--config", str(a.config), "--wide-threshold", str(a.wide_threshold)],
                               capture_output=True, text=True, timeout=a.timeout)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                return r.returncode or 1
            res[mode].append(json.loads(line[-1][7:]))
            print(f"repeat {rep} {mode}: done", flush=True)
    ev = {m: [[s["events"] for s in run["per_step"]] for run in res[m]] for m in modes}
    res["events_equal"] = all(e == ev[modes[0]][0] for m in modes for e in ev[m])
    out = Path(a.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    (out / (a.name + ".json")).write_text(json.dumps(res, indent=1) + "\n")
    first = res[modes[0]][0]
    L = [f"# configs[{a.config}], adaptive half of the step: " + ", ".join(modes), "",
         f"{first['particles']} particles, {a.steps} adaptive steps per process after {a.warmup} plain steps, {a.repeats} processes per mode, same start.",
         "`seconds` buckets of `AdaptivityDriver` (host clock), summed over the steps of a process; one column per repeat.", "",
         "| mode | download ms | host_decide ms | apply ms | mass_check ms | total ms | MB down | MB up |", "|---|---|---|---|---|---|---|---|"]
    reps = lambda f, m: " / ".join(f"{f(run):.2f}" for run in res[m])   # noqa: E731
    for m in modes:
        cell = {k: reps(lambda run, k=k: 1e3 * sum(s["seconds"][k] for s in run["per_step"]), m) for k in ("download", "host_decide", "apply", "mass_check")}
        total = reps(lambda run: 1e3 * sum(sum(s["seconds"].values()) for s in run["per_step"]), m)
        rows = res[m][0]["per_step"]
        L.append(f"| {m} | {cell['download']} | {cell['host_decide']} | {cell['apply']} | {cell['mass_check']} | {total} | "
                 f"{sum(r['bytes_device_to_host'] for r in rows) / 1e6:.1f} | {sum(r['bytes_host_to_device'] for r in rows) / 1e6:.1f} |")
    L += ["", "Per partner search (pass), first repeat's counts; ms = download + host_decide + apply of that pass, one value per repeat:", "",
          "| mode | step | pass | n | participants | exported indices | bytes down | bytes up | events | download ms | host_decide ms | apply ms |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for m in modes:
        for si, srow in enumerate(res[m][0]["per_step"]):
            for pi, ps in enumerate(srow["passes"]):
                t = {k: " / ".join(f"{1e3 * run['per_step'][si]['passes'][pi]['seconds'][k]:.2f}" for run in res[m]) for k in ("download", "host_decide", "apply")}
                L.append(f"| {m} | {srow['step_number']} | {ps['kind']} | {ps['n']} | {ps['participants']} | {ps['exported_indices']} | {ps['bytes_down']} | "
                         f"{ps['bytes_up']} | {ps['events']} | {t['download']} | {t['host_decide']} | {t['apply']} |")
    if "device" in modes:
        L += ["", "Device mode, the search of every pass (first repeat; apply ms above = classify + search + apply):", "",
              "| step | pass | K | candidates | donors | transfers | rounds | max_frontier | wide_rounds |", "|---|---|---|---|---|---|---|---|---|"]
        for srow in res["device"][0]["per_step"]:
            for ps in srow["passes"]:
                q = ps["search"]
                L.append(f"| {srow['step_number']} | {ps['kind']} | {q['participants']} | {q['candidates']} | {q['donors']} | {q['transfers']} | {q['rounds']} | "
                         f"{q['max_frontier']} | {q['wide_rounds']} |")
    L += ["", "Events per step (first repeat):", ""]
    for m in modes:
        L.append(f"- {m}: " + "; ".join(f"{s['step_number']}: {s['events']}" for s in res[m][0]["per_step"]))
    tot = {k: sum(s["events"][k] for s in first["per_step"]) for k in ("shares", "merges", "splits")}
    L += ["", f"Totals over the steps: {tot}.  Event counts equal between all modes and repeats in every step: **{res['events_equal']}**.", "",
          "Profiler scopes over two further adaptive steps (event profiler on, not part of the buckets above; first repeat):", ""]
    for m in modes:
        L.append(f"- {m}: " + (", ".join(f"{k} {v['total_ms']:.3f} ms in {v['scopes']} scopes" for k, v in sorted(res[m][0]["profiled_steps"]["scopes"].items())) or "none"))
    (out / (a.name + ".md")).write_text("\n".join(L) + "\n")
    print("\n".join(L))
    return 0 if res["events_equal"] else 2


if __name__ == "__main__":
    sys.exit(main())
