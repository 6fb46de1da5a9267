"""configs[4]'s adaptive step on slabs in the three export modes of distributed.group_single_step_adaptivity_on_slabs: every rank's whole
CSR ("lists"), the candidate rows filtered on the ranks ("candidates", include/sph_slab_candidates.h) and the compact partner problem
("compact", include/sph_slab_partner_problem.h: only the participants cross the bus, K decisions go back up).

configs[4]'s scene and parameters as scripts/gpu_slab_candidates_time.py builds them, on TWO LOOPBACK RANKS of one device, a few adaptive
steps per mode from the same start, ONE PROCESS PER MODE (fresh children of this script, one after the other, in one invocation).
`candidates` exists in the parent commit and is the baseline.  Per PASS (one partner search and its apply; a split is a pass of its
own) the wall time of its parts, taken around the calls: `prepare` (the collective prepare on the ranks), `download` (rows, problems,
fields, ids, mass sums), `assemble` (assemble_lists / merge_slab_partner_problems), `decide` (the host search), `apply`; the size of the
search (n or K) and its candidates.  Per adaptive step the bytes down / up as the driver counts them (lists and candidates mode send
6 B per particle and rank up per pass; the driver does not count that, this script adds it).  In lists mode the one export of the whole
CSR is charged to the step's first pass.  The event counts must be equal between the modes.
Writes <out-dir>/<name>.json and <name>.md.

    python scripts/gpu_slab_partner_problem_time.py [--steps 2] [--warmup 2] [--out-dir profiles] [--name r12_slab_partner_problem]
"""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
MODES = ("lists", "candidates", "compact")
PARTS = ("prepare_s", "download_s", "assemble_s", "decide_s", "apply_s")


def child(mode: str, steps: int, warmup: int) -> dict:
    import numpy as np
    import torch  # noqa: F401  (runtime load order, see ffi.load_product)
    from adaptive_sph_amd import distributed as D, ffi, scene as sc
    from adaptive_sph_amd.adaptivity import SplitPatterns
    from adaptive_sph_amd.workloads import WORKLOADS
    plib = ffi.load_product()
    scene_f, params_f, desc = WORKLOADS["ratio_stress_4m"]
    r_fine = float(np.sqrt(np.float32(0.0004385) ** 2 * 0.93 / np.pi))
    P = params_f(level_estimation_method="EmptyAngle", merging=True, sharing=True, splitting=True, particle_radius_fine=r_fine,
                 particle_radius_base=50 * r_fine, maximum_surface_distance=0.3)
    scn = scene_f()
    pos, mass, vel = sc.init_particles(scn)
    grp = D.make_loopback_group(plib, pos, mass, vel, sc.boundary_planes(scn.boundary, P.init_boundary_handler), 2)
    sp = SplitPatterns.load_from_file(REPO / "tests" / "golden" / "split-patterns.yaml")
    for c in grp:
        c.set_split_patterns(sp.patterns)
    p = P.to_ffi()
    spent = dict.fromkeys(PARTS, 0.0)
    size = {"n": 0, "candidates": 0}
    passes = []

    def close_pass(kind):
        passes.append({"kind": kind, **size, **spent})
        spent.update(dict.fromkeys(PARTS, 0.0))
        size.update(n=0, candidates=0)

    depth = [0]

    def timed(owner, name, bucket, after=None):
        inner = getattr(owner, name)

        def wrapped(*a, **kw):
            t0 = time.perf_counter()
            depth[0] += 1
            try:
                return inner(*a, **kw)
            finally:
                depth[0] -= 1
                if depth[0] == 0:   # (merge_slab_partner_problems calls assemble_lists: the outermost call owns the time)
                    spent[bucket] += time.perf_counter() - t0
                if after:
                    after(a)
        setattr(owner, name, wrapped)

    def searched_full(a):       # _decide_on_gathered(lib, kind, g, lists, P, dt)
        size.update(n=len(a[2]["mass"]), candidates=len(a[3][1]))

    def searched_compact(a):    # _decide_compact(lib, kind, ids, fields, off_c, idx_c, P, dt)
        size.update(n=len(a[2]), candidates=len(a[5]))

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
    timed(ffi, "group_adapt", "apply_s", lambda a: close_pass(a[1]))
    timed(ffi, "group_adapt_compact", "apply_s", lambda a: close_pass(a[1]))
    for _ in range(warmup):
        ffi.group_step(grp, p)
    per_step = []
    for _ in range(steps):
        sts = ffi.group_step(grp, p)
        n = sum(c.n for c in grp)
        spent.update(dict.fromkeys(PARTS, 0.0))
        passes.clear()
        t0 = time.perf_counter()
        info = D.group_single_step_adaptivity_on_slabs(plib, grp, P, float(sts[0].dt), int(sts[0].step_number), export=mode)
        wall = time.perf_counter() - t0
        searches = sum(1 for q in passes if q["kind"] != "split")
        per_step.append({"step_number": int(sts[0].step_number), "n_before": n, "n_after": info["n_after"], "adaptive_half_s": wall,
                         "passes": [dict(q) for q in passes], "participants": info.get("participants", 0), "exported_indices": info["exported_indices"],
                         "bytes_down": info["bytes_down"], "bytes_up": info.get("bytes_up", 6 * n * len(grp) * searches),
                         "events": {k: info[k] for k in ("shares", "merges", "splits")}})
    return {"mode": mode, "workload": desc, "ranks": 2, "device": torch.cuda.get_device_name(0), "per_step": per_step}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out-dir", default=str(REPO / "profiles"))
    ap.add_argument("--name", default="r12_slab_partner_problem")
    ap.add_argument("--child", choices=MODES)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(child(a.child, a.steps, a.warmup)))
        return
    res = {}
    for mode in MODES:
        r = subprocess.run([sys.executable, __file__, "--child", mode, "--steps", str(a.steps), "--warmup", str(a.warmup)], capture_output=True, text=True,
                           timeout=900)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"mode {mode} failed (exit {r.returncode})")
        res[mode] = json.loads(line[-1][7:])
        print(f"{mode}: done", flush=True)
    ev = [[s["events"] for s in res[m]["per_step"]] for m in MODES]
    assert ev[0] == ev[1] == ev[2], ("the modes took different decisions", ev)
    out = Path(a.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    (out / (a.name + ".json")).write_text(json.dumps(res, indent=1) + "\n")
    md = [f"# The compact partner problem on slabs: {res['lists']['workload']}", "",
          f"Two loopback ranks on one {res['lists']['device']}, one process per mode in one invocation, {a.warmup} plain steps, then {a.steps} adaptive steps; one run.",
          "`candidates` is the parent commit's mode and the baseline.  Seconds of wall time per pass, taken around the calls on the host.", "",
          "## Per adaptive step", "",
          "| step | events (shares / merges / splits) | mode | adaptive half | participants | candidates | bytes down | bytes up |",
          "|---|---|---|---|---|---|---|---|"]
    for k in range(len(res["lists"]["per_step"])):
        for m in MODES:
            s = res[m]["per_step"][k]
            e = s["events"]
            md.append(f"| {s['step_number']} | {e['shares']} / {e['merges']} / {e['splits']} | {m} | {s['adaptive_half_s']:.4f} | {s['participants'] or '-'} | "
                      f"{s['exported_indices']} | {s['bytes_down']} | {s['bytes_up']} |")
    md += ["", "## Per pass", "", "| step | pass | mode | size of the search (n or K) | candidates | prepare | download | assemble / merge | decide | apply |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for k in range(len(res["lists"]["per_step"])):
        for m in MODES:
            s = res[m]["per_step"][k]
            for q in s["passes"]:
                md.append(f"| {s['step_number']} | {q['kind']} | {m} | {q['n'] or '-'} | {q['candidates'] or '-'} | {q['prepare_s']:.4f} | {q['download_s']:.4f} | "
                          f"{q['assemble_s']:.4f} | {q['decide_s']:.4f} | {q['apply_s']:.4f} |")
    (out / (a.name + ".md")).write_text("\n".join(md) + "\n")
    print("\n".join(md))


if __name__ == "__main__":
    main()
