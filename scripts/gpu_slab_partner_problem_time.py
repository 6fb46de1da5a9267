"""The adaptive step on slabs in the export modes of distributed.group_single_step_adaptivity_on_slabs: every rank's whole CSR ("lists"),
the candidate rows filtered on the ranks ("candidates", include/sph_slab_candidates.h), the compact partner problem ("compact",
include/sph_slab_partner_problem.h: only the participants cross the bus, K decisions go back up) and the search on the device
("device", include/sph_slab_partner_search.h: the local problems merged and solved on member 0's device, the decisions handed over
device to device).

configs[0] (default-scene.yaml with the default configuration) and configs[4] (its scene and parameters as
scripts/gpu_slab_candidates_time.py builds them), on TWO LOOPBACK RANKS of one device, a few adaptive steps per mode from the same
start, ONE PROCESS PER MODE AND RUN (fresh children of this script, one after the other, in one invocation).  Per PASS (one partner
search and its apply; a split is a pass of its own) the wall time of its parts, taken around the calls on the host: `prepare` (the
collective prepare on the ranks), `download` (rows, problems, fields, ids, mass sums), `assemble` (assemble_lists /
merge_slab_partner_problems), `decide` (the host search), `apply`; the size of the search (n or K) and its candidates.  The device
mode's prepare, merge, search and hand-over happen inside ONE library call: `find` is the wall time of that call, and a further child
per run ("device+profile") repeats the mode with the library's marker events on and reports the device time between the markers of
the call's phases -- the prepare's scopes, slab_search_stage / mark / fields / rows (merge), search_writers / rounds / validate
(search), slab_search_handover.  Per adaptive step the bytes down / up as the driver counts them (lists and candidates mode send 6 B
per particle and rank up per pass; the driver does not count that, this script adds it).  In lists mode the one export of the whole CSR
is charged to the step's first pass.  The event counts must be equal between the modes and the runs.  Every time in the tables is the
median over the runs, with the smallest and the largest beside it.
Writes <out-dir>/<name>.json and <name>.md.

    python scripts/gpu_slab_partner_problem_time.py [--configs 0 4] [--modes compact device] [--runs 3] [--steps 2] [--warmup 2]
                                                    [--out-dir profiles] [--name r13_slab_device_search]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
MODES = ("lists", "candidates", "compact", "device", "device+profile")
PARTS = ("prepare_s", "download_s", "assemble_s", "decide_s", "find_s", "apply_s")
PHASES = ("prepare_ms", "merge_ms", "search_ms", "handover_ms")   # device+profile: the device time inside sph_group_find_partners_device


def phase_of(scope: str) -> str:
    if scope == "slab_search_handover":
        return "handover_ms"
    if scope.startswith("slab_search_"):
        return "merge_ms"
    if scope.startswith("search_"):
        return "search_ms"
    return "prepare_ms"


def setup(config: int):
    """-> (workload description, params, (pos, mass, vel, planes))"""
    import numpy as np
    from adaptive_sph_amd import scene as sc
    from adaptive_sph_amd.workloads import WORKLOADS, default_params
    if config == 0:
        P = default_params()
        scn = sc.SceneConfig.from_yaml(str(REPO / "tests" / "golden" / "default-scene.yaml"))
        desc = "configs[0]: default-scene.yaml, default configuration"
    else:
        scene_f, params_f, desc = WORKLOADS["ratio_stress_4m"]
        r_fine = float(np.sqrt(np.float32(0.0004385) ** 2 * 0.93 / np.pi))
        P = params_f(level_estimation_method="EmptyAngle", merging=True, sharing=True, splitting=True, particle_radius_fine=r_fine,
                     particle_radius_base=50 * r_fine, maximum_surface_distance=0.3)
        scn = scene_f()
        desc = "configs[4]: " + desc
    pos, mass, vel = sc.init_particles(scn)
    return desc, P, (pos, mass, vel, sc.boundary_planes(scn.boundary, P.init_boundary_handler))


def child(mode: str, config: int, steps: int, warmup: int) -> dict:
    import torch  # noqa: F401  (runtime load order, see ffi.load_product)
    from adaptive_sph_amd import distributed as D, ffi
    from adaptive_sph_amd.adaptivity import SplitPatterns
    plib = ffi.load_product()
    desc, P, (pos, mass, vel, planes) = setup(config)
    profiled = mode == "device+profile"
    export = "device" if profiled else mode
    grp = D.make_loopback_group(plib, pos, mass, vel, planes, 2)
    sp = SplitPatterns.load_from_file(REPO / "tests" / "golden" / "split-patterns.yaml")
    for c in grp:
        c.set_split_patterns(sp.patterns)
    p = P.to_ffi()
    spent = dict.fromkeys(PARTS, 0.0)
    size = {"n": 0, "candidates": 0, "rounds": 0}
    phases = dict.fromkeys(PHASES, 0.0)
    passes = []

    def close_pass(kind):
        passes.append({"kind": kind, **size, **spent, **phases})
        spent.update(dict.fromkeys(PARTS, 0.0))
        phases.update(dict.fromkeys(PHASES, 0.0))
        size.update(n=0, candidates=0, rounds=0)

    depth = [0]

    def timed(owner, name, bucket, after=None, before=None):
        inner = getattr(owner, name)

        def wrapped(*a, **kw):
            if before:
                before()
            t0 = time.perf_counter()
            depth[0] += 1
            out = None
            try:
                out = inner(*a, **kw)
                return out
            finally:
                depth[0] -= 1
                if depth[0] == 0:   # (merge_slab_partner_problems calls assemble_lists: the outermost call owns the time)
                    spent[bucket] += time.perf_counter() - t0
                if after:
                    after(a, out)
        setattr(owner, name, wrapped)

    def searched_full(a, out):       # _decide_on_gathered(lib, kind, g, lists, P, dt)
        size.update(n=len(a[2]["mass"]), candidates=len(a[3][1]))

    def searched_compact(a, out):    # _decide_compact(lib, kind, ids, fields, off_c, idx_c, P, dt)
        size.update(n=len(a[2]), candidates=len(a[5]))

    def reset_markers():
        if profiled:
            for c in grp:
                c.profile_reset()

    def found(a, out):               # group_find_partners_device(contexts, kind, p, ap, ..) -> info
        if out is None:
            return
        size.update(n=out["participants"], candidates=out["candidates"], rounds=out["rounds"])
        if profiled:
            for c in grp:
                for scope, (_, ms) in c.profile_get().items():
                    phases[phase_of(scope)] += ms

    timed(ffi.Context, "download_neighbors", "download_s")
    timed(ffi.Context, "slab_candidates_download", "download_s")
    timed(ffi.Context, "slab_partner_problem_download", "download_s")
    timed(ffi.Context, "slab_sum_mass", "download_s")
    timed(D, "gather_by_id", "download_s")
    timed(ffi, "group_slab_candidates_prepare", "prepare_s")
    timed(ffi, "group_slab_partner_problem_prepare", "prepare_s")
    timed(D, "assemble_lists", "assemble_s")
    timed(D, "merge_slab_partner_problems", "assemble_s")
    timed(D, "_decide_on_gathered", "decide_s", searched_full)
    timed(D, "_decide_compact", "decide_s", searched_compact)
    timed(ffi, "group_find_partners_device", "find_s", found, reset_markers)
    timed(ffi, "group_adapt", "apply_s", lambda a, out: close_pass(a[1]))
    timed(ffi, "group_adapt_compact", "apply_s", lambda a, out: close_pass(a[1]))
    timed(ffi, "group_adapt_device", "apply_s", lambda a, out: close_pass(a[1]))
    for _ in range(warmup):
        ffi.group_step(grp, p)
    if profiled:
        for c in grp:
            c.profile_enable(1)
    per_step = []
    for _ in range(steps):
        sts = ffi.group_step(grp, p)
        n = sum(c.n for c in grp)
        spent.update(dict.fromkeys(PARTS, 0.0))
        passes.clear()
        t0 = time.perf_counter()
        info = D.group_single_step_adaptivity_on_slabs(plib, grp, P, float(sts[0].dt), int(sts[0].step_number), export=export)
        wall = time.perf_counter() - t0
        searches = sum(1 for q in passes if q["kind"] != "split")
        per_step.append({"step_number": int(sts[0].step_number), "n_before": n, "n_after": info["n_after"], "adaptive_half_s": wall,
                         "passes": [dict(q) for q in passes], "participants": info.get("participants", 0), "exported_indices": info["exported_indices"],
                         "bytes_down": info["bytes_down"], "bytes_up": info.get("bytes_up", 6 * n * len(grp) * searches),
                         "bytes_between_devices": info.get("bytes_between_devices", 0), "events": {k: info[k] for k in ("shares", "merges", "splits")}})
    return {"mode": mode, "workload": desc, "ranks": 2, "device": torch.cuda.get_device_name(0), "per_step": per_step}


def spread(values) -> str:
    return f"{statistics.median(values):.4f} ({min(values):.4f} .. {max(values):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--configs", type=int, nargs="+", default=[0, 4], choices=(0, 4))
    ap.add_argument("--modes", nargs="+", default=["compact", "device", "device+profile"], choices=MODES)
    ap.add_argument("--out-dir", default=str(REPO / "profiles"))
    ap.add_argument("--name", default="r13_slab_device_search")
    ap.add_argument("--child", choices=MODES)
    ap.add_argument("--config", type=int, default=4)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.config, a.steps, a.warmup)))
        return
    res = {}
    for config in a.configs:
        for mode in a.modes:
            for run in range(a.runs):
                r = subprocess.run([sys.executable, __file__, "--child", mode, "--config", str(config), "--steps", str(a.steps), "--warmup", str(a.warmup)],
                                   capture_output=True, text=True, timeout=900)
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    raise SystemExit(f"configs[{config}] mode {mode} run {run} failed (exit {r.returncode})")
                res.setdefault(str(config), {}).setdefault(mode, []).append(json.loads(line[-1][7:]))
                print(f"configs[{config}] {mode} run {run}: done", flush=True)
    out = Path(a.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    (out / (a.name + ".json")).write_text(json.dumps(res, indent=1) + "\n")
    base = a.modes[0]
    md = []
    for config in a.configs:
        R = res[str(config)]
        ev = [[s["events"] for s in run["per_step"]] for m in a.modes for run in R[m]]
        assert all(e == ev[0] for e in ev), ("the modes or the runs took different decisions", ev)
        first = R[base][0]
        md += [f"## {first['workload']}", "",
               f"Two loopback ranks on one {first['device']}, one process per mode and run in one invocation, {a.warmup} plain steps, then {a.steps} adaptive steps; "
               f"{a.runs} runs per mode.  `{base}` is the baseline.  Seconds of wall time, taken around the calls on the host: the median of the runs (smallest .. largest).", "",
               "### Per adaptive step", "",
               "| step | events (shares / merges / splits) | mode | adaptive half | participants | candidates | bytes down | bytes up | bytes between devices |",
               "|---|---|---|---|---|---|---|---|---|"]
        n_steps = len(first["per_step"])
        for k in range(n_steps):
            for m in a.modes:
                runs = [run["per_step"][k] for run in R[m]]
                s, e = runs[0], runs[0]["events"]
                md.append(f"| {s['step_number']} | {e['shares']} / {e['merges']} / {e['splits']} | {m} | {spread([q['adaptive_half_s'] for q in runs])} | "
                          f"{s['participants'] or '-'} | {s['exported_indices']} | {s['bytes_down']} | {s['bytes_up']} | {s['bytes_between_devices'] or '-'} |")
        md += ["", "### Per pass (host wall time)", "",
               "| step | pass | mode | size of the search (n or K) | candidates | rounds | prepare | download | assemble / merge | decide | find (one call) | apply |",
               "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for k in range(n_steps):
            for m in a.modes:
                runs = [run["per_step"][k]["passes"] for run in R[m]]
                for j, q in enumerate(runs[0]):
                    cols = " | ".join(spread([r[j][part] for r in runs]) if any(r[j][part] for r in runs) else "-" for part in PARTS)
                    md.append(f"| {R[m][0]['per_step'][k]['step_number']} | {q['kind']} | {m} | {q['n'] or '-'} | {q['candidates'] or '-'} | {q['rounds'] or '-'} | {cols} |")
        if "device+profile" in a.modes:
            md += ["", "### Inside the device mode's one call (device time between the library's markers, milliseconds, summed over the two members)", "",
                   "| step | pass | K | prepare | merge | search | hand-over |", "|---|---|---|---|---|---|---|"]
            for k in range(n_steps):
                runs = [run["per_step"][k]["passes"] for run in R["device+profile"]]
                for j, q in enumerate(runs[0]):
                    if q["kind"] == "split":
                        continue
                    cols = " | ".join(spread([r[j][ph] for r in runs]) for ph in PHASES)
                    md.append(f"| {R['device+profile'][0]['per_step'][k]['step_number']} | {q['kind']} | {q['n']} | {cols} |")
        md.append("")
    (out / (a.name + ".md")).write_text("\n".join(md) + "\n")
    print("\n".join(md))


if __name__ == "__main__":
    main()
